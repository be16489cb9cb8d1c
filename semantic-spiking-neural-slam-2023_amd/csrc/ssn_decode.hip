// ssn_decode.hip - grid decoding of SSP trajectories behind ssn_decoder_* (include/ssn.h).
//
// Not on the step path and independent of ssn_sim: for every input row u_t (normalised as SSPSpace.decode normalises) the index
// of the table row with the largest similarity, best[t] = argmax_j sum_k u_t[k] table[j][k], lowest j on ties - the
// 'from-set' grid decode that ends every experiment (reference run_pathint.py:171-179, run_slam.py:242-268).  The T x S
// similarity matrix is never written: the product kernel's epilogue keeps one (value, column) pair per row.
//
//   k_decode_prepare   one wave per row: norm in f64 (fixed order), row / norm when norm >= 1e-6 else the row as it is, converted
//                      to the decoder's dtype, zero-padded to Kp = 32 ceil(K / 32) columns and to whole 128-row tiles.
//   k_decode_tiles     128 x 128 similarity tile per 256-thread workgroup (2 x 2 waves, 64 x 64 per wave), K in slabs through LDS
//                      with the next slab prefetched into registers (as k_gemm_nt_mfma_f32).  A workgroup walks the
//                      tiles_per_strip column tiles of its strip for its row tile; every thread keeps the running best of the
//                      rows its accumulator registers belong to (columns ascend, so a strict > keeps the lowest column), and at
//                      the end of the strip the 32 (16) lanes of a row and then the two waves beside each other are reduced with
//                      the (value, lowest column) rule: one partial per row and strip, written with plain stores - no atomics, so
//                      the answer is the same from run to run.  Both operands are padded, so no load is bounds-checked; padded
//                      columns (>= S) never enter a comparison and padded rows (>= n_rows) are never written.
//                      f32: v_mfma_f32_32x32x2_f32, 2 x 2 accumulators of 16 registers per wave, slabs of 32 - every similarity
//                      is bit for bit the k-ordered fmaf chain over the whole K, whatever the chunking, so the results do not
//                      depend on the scratch size.  f64 (parity mode): v_mfma_f64_16x16x4_f64, 4 x 4 accumulators, slabs of 16.
//                      Tile and occupancy: 128 x 128 x 32 (f64: x 16) per workgroup of 4 waves, one wave per SIMD, two workgroups
//                      per CU asked for with __launch_bounds__(256, 2) - the second hides the first's barriers and slab loads; a
//                      wave's four accumulators are independent, which is what the 64-cycle MFMA needs to issue back to back.
//                      tools/kernel_resources.py ssn_decode.hip k_decode_tiles:  f32 253 VGPR (64 accumulator, 64 running best,
//                      32 prefetch), 0 AGPR, no scratch, LDS 35 840 B, occupancy 2;  f64 256 VGPR + 158 AGPR, LDS 37 888 B,
//                      occupancy 1.  One k step of a wave is 4 LDS reads for 4 MFMAs (f64: 8 for 16).
//   k_decode_finish    one wave per row: the partials of its strips in column order, same rule -> int32 best; the similarity to
//                      that sample accumulated again in f64.
//   k_decode_map       the storing twin of k_decode_tiles behind ssn_decoder_map: the same tile walk - operands, Kp
//                      padding, slab order and MFMA sequence, over the tiles_per_run column tiles of a run instead of a strip - so
//                      every entry is the accumulator value k_decode_tiles compares; after each tile's K loop the tile itself - s,
//                      or s * s (one multiply in T) - is stored at out[(t0 + r) out_ld + col] for rows < n_rows and columns < S,
//                      in T or widened to double.  No running best, no LDS reduction, no finish kernel.
//                      tools/kernel_resources.py ssn_decode.hip k_decode_map:  f32 250 VGPR (64 accumulator, 32 prefetch, the rest
//                      hoisted store addresses), 0 AGPR, no scratch, LDS 33 792 B, occupancy 2;  f64 254 VGPR + 140 AGPR, LDS
//                      34 816 B, occupancy 1.  Store form: plain dword stores, an accumulator register of a wave being 32
//                      consecutive columns of two rows (two 128-B segments; f64: four rows of 16 doubles); with a device output the
//                      kernel costs what k_decode_tiles + k_decode_finish cost on the same rows (0.49 against 0.52 ms at 2 000 x
//                      1015 over 100 x 100, 3.7 against 4.1 ms at 20 000 rows), so the LDS-transposed 16-byte store was not built:
//                      it had no time left to recover.  k_decode_prepare<.., SCALE = false> feeds it the raw rows of normalize=False.
//
// Scratch (fixed at creation, default 64 MB): per row K doubles of upload staging, Kp converted values, one (value, column)
// partial per strip slot and the (double similarity, best) result.  The host cuts n_rows into chunks of whole row tiles that fit and the
// column walk into at most `slots` strips (ssn_decoder::plan: cut_rows, tiles_per_part); the smallest scratch holds one row tile with
// one strip.  The error reporting, the device guard and the Lane (device check, stream, events, scratch area) are
// csrc/ssn_service.hpp's, shared with the encoder and the binder.
//
// The table comes from the host (ssn_decoder_create: converted and uploaded) or is made here from the sample points
// (ssn_decoder_create_from_points: a float64 ssn_encoder of csrc/ssn_encode.hip writes it chunk by chunk in the decoder's dtype).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
#include "../../include/ssn.h"
#include "ssn_encode.hpp"       // encoder_encode_into: the table of ssn_decoder_create_from_points
#include "ssn_kernels.hpp"      // launch_gemm_nt / launch_argmax_partial: the materialising composition ssn_decoder_rows_composed times
#include "ssn_service.hpp"

using namespace ssn::svc;      // fail, SVC_HIP, DevGuard, Lane, elapsed, stage_rows, check_rows

namespace {

constexpr int TILE = 128;            // rows and columns of a workgroup's similarity tile
constexpr int KPAD = 32;             // operands are padded to a multiple of this many columns
constexpr int MAX_SLOTS = 64;        // strips per row chunk at most

template <typename T> struct Mma;
template <> struct Mma<float> {
  static constexpr int MT = 32, KS = 2, AR = 16, BK = 32;
  typedef float acc_t __attribute__((ext_vector_type(16)));
  static __device__ __forceinline__ int lane_mn(int l) { return l & 31; }
  static __device__ __forceinline__ int lane_k(int l) { return l >> 5; }
  static __device__ __forceinline__ int acc_row(int v, int l) { return (v & 3) + 8 * (v >> 2) + 4 * (l >> 5); }
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};
template <> struct Mma<double> {
  static constexpr int MT = 16, KS = 4, AR = 4, BK = 16;
  typedef double acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ int lane_mn(int l) { return l & 15; }
  static __device__ __forceinline__ int lane_k(int l) { return l >> 4; }
  static __device__ __forceinline__ int acc_row(int v, int l) { return (l >> 4) + 4 * v; }
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
};

// (value, column) candidates: the larger value wins, the lower column on equal values
template <typename T>
__device__ __forceinline__ void take_better(T& bv, int& bc, T v, int c) {
  if (v > bv || (v == bv && c < bc)) { bv = v; bc = c; }
}

// SCALE = false (the raw rows of a map with normalize off) leaves out the norm: the rows are only converted and padded
template <typename TI, typename T, bool SCALE = true>
__global__ __launch_bounds__(256) void k_decode_prepare(const TI* __restrict__ src, long long ld, int n_rows, int n_pad_rows, int K, int Kp,
                                                        T* __restrict__ dst) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_pad_rows) return;
  T* d = dst + (size_t)row * Kp;
  if (row >= n_rows) {
    for (int k = lane; k < Kp; k += 64) d[k] = T(0);
    return;
  }
  const TI* s = src + (size_t)row * ld;
  double nrm = 1.0;
  bool scale = false;
  if constexpr (SCALE) {
    double ss = 0.0;
    for (int k = lane; k < K; k += 64) { const double x = (double)s[k]; ss += x * x; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    nrm = sqrt(ss);
    scale = nrm >= 1e-6;
  }
  for (int k = lane; k < Kp; k += 64) {
    double x = 0.0;
    if (k < K) { x = (double)s[k]; if (scale) x = x / nrm; }
    d[k] = (T)x;
  }
}

template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 2 : 1) void k_decode_tiles(const T* __restrict__ rows, const T* __restrict__ table, int Kp, int n_rows, unsigned S,
                                                      int col_tiles, int tiles_per_strip, T* __restrict__ pval, int* __restrict__ pcol,
                                                      int part_ld) {
  using M = Mma<T>;
  constexpr int BK = M::BK, LD = BK + 1, MT = M::MT, NI = 64 / MT, AR = M::AR, KS = M::KS;
  constexpr int RS = 256 / BK, RPT = TILE / RS;      // this thread stages rows lr + RS i, column lc of a slab
  __shared__ T As[TILE][LD];
  __shared__ T Ws[TILE][LD];
  __shared__ T red_v[2][TILE];
  __shared__ int red_c[2][TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int t0 = blockIdx.x * TILE;
  const int ct0 = blockIdx.y * tiles_per_strip, ct1 = min(ct0 + tiles_per_strip, col_tiles);
  const int lr = tid / BK, lc = tid % BK;
  // uniform tile bases + one 32-bit lane offset: the row offsets RS i Kp of the slab loads stay in scalar registers
  const T* __restrict__ a0 = rows + (size_t)t0 * Kp;
  const unsigned voff = (unsigned)lr * (unsigned)Kp + (unsigned)lc;      // < 128 Kp <= 2^27
  T ra[RPT], rw[RPT];
  auto fetch = [&](int ct, int k0) {
    const T* a = a0 + k0;
    const T* w = table + (size_t)ct * TILE * Kp + k0;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const unsigned o = (unsigned)(RS * i) * (unsigned)Kp;
      ra[i] = (a + o)[voff];
      rw[i] = (w + o)[voff];
    }
  };
  T bv[NI * AR];
  int bc[NI * AR];
#pragma unroll
  for (int s = 0; s < NI * AR; ++s) { bv[s] = T(-INFINITY); bc[s] = ct0 * TILE; }      // a real column, whatever the input holds
  const int mn = M::lane_mn(lane);
  const T* ap = &As[wm * 64 + mn][M::lane_k(lane)];
  const T* wp = &Ws[wn * 64 + mn][M::lane_k(lane)];
  fetch(ct0, 0);
  for (int ct = ct0; ct < ct1; ++ct) {
    typename M::acc_t acc[NI][NI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int v = 0; v < AR; ++v) acc[i][j][v] = T(0);
    for (int k0 = 0; k0 < Kp; k0 += BK) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) { As[lr + RS * i][lc] = ra[i]; Ws[lr + RS * i][lc] = rw[i]; }
      __syncthreads();
      if (k0 + BK < Kp) fetch(ct, k0 + BK);
      else if (ct + 1 < ct1) fetch(ct + 1, 0);
#pragma unroll 4
      for (int kk = 0; kk < BK; kk += KS) {
        T a[NI], b[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) { a[i] = ap[i * MT * LD + kk]; b[i] = wp[i * MT * LD + kk]; }
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j) acc[i][j] = M::mma(a[i], b[j], acc[i][j]);
      }
      __syncthreads();
    }
    // epilogue of the tile: columns ascend with j and with ct, so a strict > keeps the lowest column of a tie
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const unsigned col = (unsigned)ct * TILE + wn * 64 + j * MT + mn;
      if (col < S) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int v = 0; v < AR; ++v)
            if (acc[i][j][v] > bv[i * AR + v]) { bv[i * AR + v] = acc[i][j][v]; bc[i * AR + v] = (int)col; }
      }
    }
  }
  // the MT lanes that hold one row, then the two waves side by side
#pragma unroll
  for (int s = 0; s < NI * AR; ++s) {
#pragma unroll
    for (int off = 1; off < MT; off <<= 1) {
      const T ov = __shfl_xor(bv[s], off, 64);
      const int oc = __shfl_xor(bc[s], off, 64);
      take_better(bv[s], bc[s], ov, oc);
    }
  }
  if (mn == 0) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int v = 0; v < AR; ++v) {
        const int r = wm * 64 + i * MT + M::acc_row(v, lane);
        red_v[wn][r] = bv[i * AR + v];
        red_c[wn][r] = bc[i * AR + v];
      }
  }
  __syncthreads();
  if (tid < TILE && t0 + tid < n_rows) {
    T v = red_v[0][tid];
    int c = red_c[0][tid];
    take_better(v, c, red_v[1][tid], red_c[1][tid]);
    pval[(size_t)blockIdx.y * part_ld + t0 + tid] = v;
    pcol[(size_t)blockIdx.y * part_ld + t0 + tid] = c;
  }
}

// k_decode_tiles' walk, copied up to the epilogue on purpose.  One force-inlined body for both (if constexpr on a store flag; outputs as
// parameters or as a struct; __restrict__ kept or dropped; plain inline) compiles to the same resources, except k_decode_tiles<double>: 158
// -> 156 AGPR.  k_decode_tiles' own text behind a force-inlined call does the same, so no shared body reproduces the registers above.
template <typename T, typename TO>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 2 : 1) void k_decode_map(const T* __restrict__ rows, const T* __restrict__ table, int Kp, int n_rows, unsigned S,
                                                      int col_tiles, int tiles_per_run, int square, TO* __restrict__ out, long long out_ld) {
  using M = Mma<T>;
  constexpr int BK = M::BK, LD = BK + 1, MT = M::MT, NI = 64 / MT, AR = M::AR, KS = M::KS;
  constexpr int RS = 256 / BK, RPT = TILE / RS;
  __shared__ T As[TILE][LD];
  __shared__ T Ws[TILE][LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int t0 = blockIdx.x * TILE;
  const int ct0 = blockIdx.y * tiles_per_run, ct1 = min(ct0 + tiles_per_run, col_tiles);
  const int lr = tid / BK, lc = tid % BK;
  const T* __restrict__ a0 = rows + (size_t)t0 * Kp;
  const unsigned voff = (unsigned)lr * (unsigned)Kp + (unsigned)lc;
  T ra[RPT], rw[RPT];
  auto fetch = [&](int ct, int k0) {
    const T* a = a0 + k0;
    const T* w = table + (size_t)ct * TILE * Kp + k0;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const unsigned o = (unsigned)(RS * i) * (unsigned)Kp;
      ra[i] = (a + o)[voff];
      rw[i] = (w + o)[voff];
    }
  };
  const int mn = M::lane_mn(lane);
  const T* ap = &As[wm * 64 + mn][M::lane_k(lane)];
  const T* wp = &Ws[wn * 64 + mn][M::lane_k(lane)];
  fetch(ct0, 0);
  for (int ct = ct0; ct < ct1; ++ct) {
    typename M::acc_t acc[NI][NI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int v = 0; v < AR; ++v) acc[i][j][v] = T(0);
    for (int k0 = 0; k0 < Kp; k0 += BK) {
#pragma unroll
      for (int i = 0; i < RPT; ++i) { As[lr + RS * i][lc] = ra[i]; Ws[lr + RS * i][lc] = rw[i]; }
      __syncthreads();
      if (k0 + BK < Kp) fetch(ct, k0 + BK);
      else if (ct + 1 < ct1) fetch(ct + 1, 0);
#pragma unroll 4
      for (int kk = 0; kk < BK; kk += KS) {
        T a[NI], b[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) { a[i] = ap[i * MT * LD + kk]; b[i] = wp[i * MT * LD + kk]; }
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j) acc[i][j] = M::mma(a[i], b[j], acc[i][j]);
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const unsigned col = (unsigned)ct * TILE + wn * 64 + j * MT + mn;
      if (col < S) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int v = 0; v < AR; ++v) {
            const int r = t0 + wm * 64 + i * MT + M::acc_row(v, lane);
            if (r < n_rows) {
              T s = acc[i][j][v];
              if (square) s = s * s;
              out[(size_t)r * (size_t)out_ld + col] = (TO)s;
            }
          }
      }
    }
  }
}

// One wave per row.  The reported similarity is not the f32 chain that won the comparison: it is accumulated again in f64 over the
// same (converted) operands, lanes striding k and a fixed butterfly.  A chain of K same-sign products - a row against its own best
// sample - drifts by up to ~3 sqrt(K) / 12 ulp, 6.6e-7 at K = 201, which is more than the 1.5e-7 sum |a b| an MFMA product is
// quoted at and more than half the decoder's bar; one extra dot product per row costs nothing next to the S it replaces.
template <typename T>
__global__ __launch_bounds__(256) void k_decode_finish(const T* __restrict__ pval, const int* __restrict__ pcol, int part_ld, int n_strips,
                                                       int n_rows, const T* __restrict__ rows, const T* __restrict__ table, int Kp,
                                                       double* __restrict__ sims, int* __restrict__ best) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  T v = pval[r];
  int c = pcol[r];
  for (int p = 1; p < n_strips; ++p) take_better(v, c, pval[(size_t)p * part_ld + r], pcol[(size_t)p * part_ld + r]);
  const T* __restrict__ u = rows + (size_t)r * Kp;
  const T* __restrict__ w = table + (size_t)c * Kp;
  double acc = 0.0;
  for (int k = lane; k < Kp; k += 64) acc = fma((double)u[k], (double)w[k], acc);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) { sims[r] = acc; best[r] = c; }
}

// ---- sub-grid refinement of the grid decode (ssn_decoder_refine_rows*) -------------------------------------------------------
// The rule, which SSPSpace.decode(method='grid-refine') follows in float64 NumPy:
//   setup   u = the row scaled as above;  c_k + i s_k = w_k fft(u)_k over the K bins of ssn_decoder_set_refine (half spectrum,
//           w = 1/d, 2/d, 2/d ..., when the phase matrix is conjugate-symmetric, else all d bins with w = 1/d);  M = phase_matrix /
//           length_scale;  x0 = points[best], the grid argmax;  box = [max(lo, x0 - pitch), min(hi, x0 + pitch)] per axis.
//   f(x)    = sum_k c_k cos(th_k) + s_k sin(th_k),  th_k = M_k . x          ( = <encode(x), u> )
//   g_a     = sum_k M_ka (s_k cos th_k - c_k sin th_k),    (-H)_ab = sum_k M_ka M_kb (c_k cos th_k + s_k sin th_k)
//   step    (exactly `iterations` of them; no data-dependent exit and no comparison of values of f, which f32 cannot rank at a
//           maximum)  Cholesky of -H, pivot j = (-H)_jj - sum_{i<j} L_ji^2;  when every pivot exceeds 1e-6 max_i (-H)_ii:
//           p = (-H)^-1 g;  otherwise p = g / max_i |H_ii| (0 when that is 0);  x <- min(max(x + p, box lo), box hi).
//   output  x;  f(x);  status bit 1: x on a box face, 2: -H not positive definite by that test at x, 4: the last step moved some
//           axis by more than 1e-6 pitch.  iterations == 0 gives points[best] exactly; an axis whose value still is the rounding of
//           x0 to the decoder's dtype reports x0 itself, so a zero row returns x0.
// Spectrum: the scaled, padded rows of k_decode_prepare times the (2K x Kp) table with w folded in, (Re, Im) interleaved:
// launch_gemm_nt<float> with one split (every entry the k-ordered fmaf chain over Kp), k_decode_spectrum in f64.
// k_decode_refine<T, DIM>: one wave64 per row, lane l owns bins l, l + 64, ...; up to REFINE_CAP bins per lane (K <= 512, d = 1015
// has 508) stay in registers with their M rows, above that they are read again from the spectrum area every step.  th is an fma
// chain in axis order, sincosf / sincos with full range reduction (|th| reaches hundreds of radians), 1 + DIM + DIM (DIM + 1) / 2
// partial sums per lane in bin order, one xor butterfly (both partners add the same two values, so every lane holds the same
// bits), and the small solve redundantly in every lane.  No atomics, no LDS.  tools/kernel_resources.py ssn_decode.hip
// k_decode_refine: f32 125 / 130 / 204 VGPR for DIM 1 / 2 / 3, f64 188 / 250 / 254, no AGPR, no scratch (the slow path of the range
// reduction stays in registers), no spills, occupancy 2 - 4.
constexpr int REFINE_CAP = 8;

__device__ __forceinline__ void sin_cos(float t, float* s, float* c) { sincosf(t, s, c); }
__device__ __forceinline__ void sin_cos(double t, double* s, double* c) { sincos(t, s, c); }

template <typename T>
__global__ __launch_bounds__(256) void k_decode_spectrum(const T* __restrict__ rows, const T* __restrict__ dft, int Kp, int N, T* __restrict__ spec) {
  const int j = blockIdx.y * 256 + threadIdx.x;
  if (j >= N) return;
  const T* __restrict__ u = rows + (size_t)blockIdx.x * Kp;
  const T* __restrict__ w = dft + (size_t)j * Kp;
  T acc = T(0);
  for (int k = 0; k < Kp; ++k) acc = fma(u[k], w[k], acc);
  spec[(size_t)blockIdx.x * N + j] = acc;
}

// one bin into the partial sums: acc[0] = f, acc[1 ..] = g, then the upper triangle of -H row by row
template <typename T, int DIM>
__device__ __forceinline__ void refine_bin(T c, T s, const T* m, const T* x, T* acc) {
  T th = m[0] * x[0];
#pragma unroll
  for (int a = 1; a < DIM; ++a) th = fma(m[a], x[a], th);
  T sn, cs;
  sin_cos(th, &sn, &cs);
  const T v = fma(c, cs, s * sn), dv = fma(s, cs, -(c * sn));
  acc[0] += v;
  int q = 1 + DIM;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    acc[1 + a] = fma(m[a], dv, acc[1 + a]);
#pragma unroll
    for (int b = a; b < DIM; ++b) { acc[q] = fma(m[a] * m[b], v, acc[q]); ++q; }
  }
}

// the step from the reduced sums; returns whether -H passed the Cholesky test
template <typename T, int DIM>
__device__ __forceinline__ bool refine_step(const T* acc, T* p) {
  T A[DIM][DIM], L[DIM][DIM];
  int q = 1 + DIM;
#pragma unroll
  for (int a = 0; a < DIM; ++a)
#pragma unroll
    for (int b = a; b < DIM; ++b) { A[a][b] = acc[q]; A[b][a] = acc[q]; ++q; }
  T dmax = A[0][0], amax = fabs(A[0][0]);
#pragma unroll
  for (int a = 1; a < DIM; ++a) { dmax = fmax(dmax, A[a][a]); amax = fmax(amax, fabs(A[a][a])); }
  bool pd = dmax > T(0);
  const T floor_ = T(1e-6) * dmax;
#pragma unroll
  for (int j = 0; j < DIM; ++j) {
    T piv = A[j][j];
#pragma unroll
    for (int i = 0; i < j; ++i) piv = fma(-L[j][i], L[j][i], piv);
    if (!(piv > floor_)) pd = false;
    const T ljj = sqrt(pd ? piv : T(1));
    L[j][j] = ljj;
#pragma unroll
    for (int r = j + 1; r < DIM; ++r) {
      T v = A[r][j];
#pragma unroll
      for (int i = 0; i < j; ++i) v = fma(-L[r][i], L[j][i], v);
      L[r][j] = v / ljj;
    }
  }
  if (pd) {
    T y[DIM];
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      T v = acc[1 + j];
#pragma unroll
      for (int i = 0; i < j; ++i) v = fma(-L[j][i], y[i], v);
      y[j] = v / L[j][j];
    }
#pragma unroll
    for (int j = DIM - 1; j >= 0; --j) {
      T v = y[j];
#pragma unroll
      for (int i = j + 1; i < DIM; ++i) v = fma(-L[i][j], p[i], v);
      p[j] = v / L[j][j];
    }
  } else {
#pragma unroll
    for (int a = 0; a < DIM; ++a) p[a] = amax > T(0) ? acc[1 + a] / amax : T(0);
  }
  return pd;
}

template <typename T, int DIM>
__global__ __launch_bounds__(256) void k_decode_refine(const T* __restrict__ spec, int K, const T* __restrict__ Mt, const double* __restrict__ points,
                                                       const int* __restrict__ best, const double* __restrict__ box, int n_rows, int iterations,
                                                       double* __restrict__ xout, double* __restrict__ fout, int* __restrict__ status) {
  constexpr int NS = 1 + DIM + DIM * (DIM + 1) / 2;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const T* __restrict__ sp = spec + (size_t)row * 2 * K;
  const bool in_regs = K <= 64 * REFINE_CAP;
  T c[REFINE_CAP], s[REFINE_CAP], m[REFINE_CAP][DIM];
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < REFINE_CAP; ++j) {
      const int k = lane + 64 * j;
      const bool ok = k < K;
      c[j] = ok ? sp[2 * k] : T(0);
      s[j] = ok ? sp[2 * k + 1] : T(0);
#pragma unroll
      for (int a = 0; a < DIM; ++a) m[j][a] = ok ? Mt[(size_t)k * DIM + a] : T(0);
    }
  }
  const size_t b = (size_t)best[row];
  double x0[DIM], lo_d[DIM], hi_d[DIM];
  T x[DIM], lo[DIM], hi[DIM], tol[DIM], last[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    x0[a] = points[b * DIM + a];
    const double pitch = box[2 * DIM + a];
    lo_d[a] = fmax(box[a], x0[a] - pitch);
    hi_d[a] = fmin(box[DIM + a], x0[a] + pitch);
    x[a] = (T)x0[a]; lo[a] = (T)lo_d[a]; hi[a] = (T)hi_d[a];
    tol[a] = (T)(1e-6 * pitch);
    last[a] = T(0);
  }
  T fval = T(0);
  bool pd = false;
  for (int it = 0;; ++it) {
    T acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = T(0);
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < REFINE_CAP; ++j) refine_bin<T, DIM>(c[j], s[j], m[j], x, acc);
    } else {
      for (int k = lane; k < K; k += 64) {
        T mk[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) mk[a] = Mt[(size_t)k * DIM + a];
        refine_bin<T, DIM>(sp[2 * k], sp[2 * k + 1], mk, x, acc);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int q = 0; q < NS; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
    T p[DIM];
    pd = refine_step<T, DIM>(acc, p);
    fval = acc[0];
    if (it >= iterations) break;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const T xn = fmin(fmax(x[a] + p[a], lo[a]), hi[a]);
      last[a] = xn - x[a];
      x[a] = xn;
    }
  }
  if (lane == 0) {
    int st = pd ? 0 : 2;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      if (x[a] <= lo[a] || x[a] >= hi[a]) st |= 1;
      if (fabs(last[a]) > tol[a]) st |= 4;
      const double xa = x[a] == (T)x0[a] ? x0[a] : (double)x[a];
      xout[(size_t)row * DIM + a] = fmin(fmax(xa, lo_d[a]), hi_d[a]);
    }
    fout[row] = (double)fval;
    status[row] = st;
  }
}

struct Plan {
  int64_t chunk_tiles, n_chunks, slots, n_strips, tiles_per_strip;
};

// t_tiles row tiles in chunks of at most `cap`: as few chunks as that allows, of even size; returns the tiles per chunk
int64_t cut_rows(int64_t t_tiles, int64_t cap, int64_t* n_chunks = nullptr) {
  const int64_t n = (t_tiles + cap - 1) / cap, chunk_tiles = (t_tiles + n - 1) / n;
  if (n_chunks) *n_chunks = (t_tiles + chunk_tiles - 1) / chunk_tiles;      // even chunks may be fewer
  return chunk_tiles;
}

// Column tiles per part - a strip of k_decode_tiles, a run of k_decode_map.  Both kernels keep two workgroups per CU resident, and
// a launch of chunk_tiles x parts workgroups runs in ceil(workgroups / resident) rounds of that many tiles each.  Of the lengths
// that make at most max_parts parts, the one that wastes the least of those rounds (the shortest on ties: more, smaller workgroups
// even out better).
int64_t tiles_per_part(int64_t col_tiles, int64_t max_parts, int64_t chunk_tiles, int64_t resident) {
  int64_t best = 0;
  double best_cost = 0.0;
  for (int64_t t = (col_tiles + max_parts - 1) / max_parts; t <= col_tiles; ++t) {
    const int64_t parts = (col_tiles + t - 1) / t, rounds = (chunk_tiles * parts + resident - 1) / resident;
    const double cost = (double)rounds * (double)t;
    if (!best || cost < best_cost) { best_cost = cost; best = t; }
    if (rounds == 1) break;      // longer parts only make the single round longer
  }
  return best;
}

}  // namespace

struct ssn_decoder : Lane {
  int dtype = 0, n_cu = 1;
  int64_t S = 0, K = 0, Kp = 0, col_tiles = 0;
  size_t esz = 4;
  void* table = nullptr;
  double kernel_ms = 0.0;          // of the last ssn_decoder_rows* call
  // refinement (ssn_decoder_set_refine): buffers of its own, beside the scratch area, so the plan stays what it was
  int r_dim = 0;
  int64_t r_K = 0, r_rows = 0;     // bins; rows the work area holds
  void *r_dft = nullptr, *r_M = nullptr;      // (2 r_K x Kp) table with w folded in, (r_K x r_dim) phases, both in the decoder's dtype
  double *r_points = nullptr, *r_box = nullptr;      // (S x r_dim) sample points; lo, hi, pitch (r_dim each)
  char* r_work = nullptr;          // per row: 2 r_K spectrum values, r_dim + 1 doubles (x, f), one status word
  // staging of host map outputs (ssn_decoder_map): a device area and pinned host memory of the same size, made on first use
  int64_t m_stage_bytes = 0, m_alloc = 0;      // asked for (0 = default_map_stage()); allocated
  char *m_dev = nullptr, *m_pin = nullptr;

  void drop_map_stage() {
    if (m_dev) (void)hipFree(m_dev);
    if (m_pin) (void)hipHostFree(m_pin);
    m_dev = m_pin = nullptr;
    m_alloc = 0;
  }
  int64_t min_map_stage(size_t out_esz) const { return TILE * S * (int64_t)out_esz; }      // one row tile of the map
  int64_t default_map_stage() const { return std::max<int64_t>((int64_t)64 << 20, min_map_stage(8)); }

  void drop_refine() {
    for (void* p : {r_dft, r_M, (void*)r_points, (void*)r_box, (void*)r_work}) if (p) (void)hipFree(p);
    r_dft = r_M = nullptr; r_points = r_box = nullptr; r_work = nullptr;
    r_dim = 0; r_K = r_rows = 0;
  }

  int64_t row_bytes(int64_t slots) const { return K * 8 + Kp * (int64_t)esz + slots * (int64_t)(esz + 4) + 12; }
  int64_t min_scratch() const { return TILE * row_bytes(1); }

  Plan plan(int64_t n_rows) const {
    Plan p;
    const int64_t t_tiles = std::max<int64_t>(1, (n_rows + TILE - 1) / TILE);
    p.slots = std::min<int64_t>(col_tiles, MAX_SLOTS);
    int64_t cap = scratch_bytes / (TILE * row_bytes(p.slots));
    if (cap < 1) {      // one row tile; as many strip slots as are left beside it
      cap = 1;
      p.slots = (scratch_bytes / TILE - row_bytes(0)) / (int64_t)(esz + 4);
    }
    cap = std::min<int64_t>(cap, (1 << 24) / TILE);
    p.chunk_tiles = cut_rows(t_tiles, cap, &p.n_chunks);
    p.tiles_per_strip = tiles_per_part(col_tiles, std::max<int64_t>(1, std::min(p.slots, col_tiles)), p.chunk_tiles, 2 * (int64_t)n_cu);      // a slot per strip
    p.n_strips = (col_tiles + p.tiles_per_strip - 1) / p.tiles_per_strip;
    return p;
  }

  ~ssn_decoder() {
    DevGuard g(device);
    drop_refine();
    drop_map_stage();
    if (table) (void)hipFree(table);
  }
};

namespace {

template <typename T>
int upload_table(ssn_decoder* d, const double* table) {
  const int64_t Sp = d->col_tiles * TILE, Kp = d->Kp, K = d->K;
  SVC_HIP(hipMalloc(&d->table, (size_t)Sp * Kp * sizeof(T)));
  SVC_HIP(hipMemset(d->table, 0, (size_t)Sp * Kp * sizeof(T)));
  const int64_t per = std::max<int64_t>(1, (int64_t)(8 << 20) / Kp);
  std::vector<T> stage((size_t)std::min(per, d->S) * Kp, T(0));
  for (int64_t r0 = 0; r0 < d->S; r0 += per) {
    const int64_t n = std::min(per, d->S - r0);
    for (int64_t r = 0; r < n; ++r) {
      const double* s = table + (size_t)(r0 + r) * K;
      T* o = stage.data() + (size_t)r * Kp;
      for (int64_t k = 0; k < K; ++k) o[k] = (T)s[k];
    }
    SVC_HIP(hipMemcpy((T*)d->table + (size_t)r0 * Kp, stage.data(), (size_t)n * Kp * sizeof(T), hipMemcpyHostToDevice));
  }
  return SSN_OK;
}

template <typename T>
struct Areas {      // the regions of the scratch area for a chunk capacity of `rows` rows and `slots` strips
  double* stage; T* conv; T* pval; int* pcol; double* sims; int* best;
  Areas(const ssn_decoder* d, int64_t rows, int64_t slots) {
    char* p = d->scratch;
    stage = (double*)p; p += (size_t)rows * d->K * 8;
    conv = (T*)p; p += (size_t)rows * d->Kp * sizeof(T);
    pval = (T*)p; p += (size_t)rows * slots * sizeof(T);
    pcol = (int*)p; p += (size_t)rows * slots * 4;
    sims = (double*)p; p += (size_t)rows * 8;
    best = (int*)p;
  }
};

template <typename T, typename TI>
hipError_t launch_prepare(ssn_decoder* d, const TI* src, int64_t ld, int n, int n_pad, T* conv, bool scale) {
  hipLaunchKernelGGL((scale ? k_decode_prepare<TI, T, true> : k_decode_prepare<TI, T, false>), dim3((unsigned)((n_pad + 3) / 4)), dim3(256), 0, d->stream, src,
                     (long long)ld, n, n_pad, (int)d->K, (int)d->Kp, conv);
  return hipGetLastError();
}

// The start of a chunk, rows [r0, r0 + n) of a call.  Rows: host doubles (dense, width K), copied to the staging area first, or
// device rows of dtype rows_dtype with leading dimension ld, read where they are.  Records ev[0] - after the upload, so the timed span
// holds kernels only - and launches k_decode_prepare into a.conv, scaling the rows or not.
template <typename T>
int prepare_chunk(ssn_decoder* d, const Areas<T>& a, const double* host, const void* dev, int rows_dtype, int64_t ld, int64_t r0, int n, int n_pad,
                  bool scale) {
  if (host)
    if (const int rc = stage_rows(d->stream, a.stage, host + (size_t)r0 * d->K, d->K, d->K, 8, n)) return rc;
  SVC_HIP(hipEventRecord(d->ev[0], d->stream));
  if (host) SVC_HIP(launch_prepare<T>(d, (const double*)a.stage, d->K, n, n_pad, a.conv, scale));
  else if (rows_dtype == SSN_F32) SVC_HIP(launch_prepare<T>(d, (const float*)dev + (size_t)r0 * ld, ld, n, n_pad, a.conv, scale));
  else SVC_HIP(launch_prepare<T>(d, (const double*)dev + (size_t)r0 * ld, ld, n, n_pad, a.conv, scale));
  return SSN_OK;
}

struct RefineOut {      // host arrays of ssn_decoder_refine_rows*; f and status may be null
  int iterations;
  double* x;
  double* f;
  int32_t* status;
};

template <typename T>
struct RefineAreas {      // the regions of the refiner's work area for `rows` rows
  T* spec; double* x; double* f; int* status;
  RefineAreas(const ssn_decoder* d, int64_t rows) {
    char* p = d->r_work;
    x = (double*)p; p += (size_t)rows * d->r_dim * 8;
    f = (double*)p; p += (size_t)rows * 8;
    spec = (T*)p; p += (size_t)rows * 2 * d->r_K * sizeof(T);
    status = (int*)p;
  }
  static size_t bytes(const ssn_decoder* d, int64_t rows) { return (size_t)rows * ((size_t)d->r_dim * 8 + 8 + 2 * (size_t)d->r_K * sizeof(T) + 4); }
};

template <typename T, int DIM>
hipError_t launch_refine(ssn_decoder* d, const RefineAreas<T>& ra, const int* best, int n, int iterations) {
  hipLaunchKernelGGL((k_decode_refine<T, DIM>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, d->stream, (const T*)ra.spec, (int)d->r_K, (const T*)d->r_M,
                     (const double*)d->r_points, best, (const double*)d->r_box, n, iterations, ra.x, ra.f, ra.status);
  return hipGetLastError();
}

// the spectrum of the prepared rows of a chunk, then the Newton steps from the chunk's grid argmax
template <typename T>
hipError_t refine_chunk(ssn_decoder* d, const RefineAreas<T>& ra, const T* conv, const int* best, int n, int iterations) {
  hipError_t e;
  if constexpr (sizeof(T) == 4) {
    e = ssn::launch_gemm_nt<float>(d->stream, conv, (int)d->Kp, (const float*)d->r_dft, (int)d->Kp, ra.spec, (int)(2 * d->r_K), n, (int)(2 * d->r_K), (int)d->Kp, 1);
  } else {
    hipLaunchKernelGGL((k_decode_spectrum<T>), dim3((unsigned)n, (unsigned)((2 * d->r_K + 255) / 256)), dim3(256), 0, d->stream, conv, (const T*)d->r_dft,
                       (int)d->Kp, (int)(2 * d->r_K), ra.spec);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return e;
  return d->r_dim == 1 ? launch_refine<T, 1>(d, ra, best, n, iterations) : d->r_dim == 2 ? launch_refine<T, 2>(d, ra, best, n, iterations)
                                                                                         : launch_refine<T, 3>(d, ra, best, n, iterations);
}

// rows: host doubles (dense, width K) or device rows of dtype rows_dtype with leading dimension ld; ro: also refine (best may be null then)
template <typename T>
int decode_rows(ssn_decoder* d, const double* host, const void* dev, int rows_dtype, int64_t ld, int64_t n_rows, int32_t* best, double* sims,
                const RefineOut* ro = nullptr) {
  DevGuard g(d->device);
  const Plan p = d->plan(n_rows);
  const int64_t cap_rows = p.chunk_tiles * TILE;
  const Areas<T> a(d, cap_rows, p.slots);
  if (ro && d->r_rows < cap_rows) {      // the work area follows the row chunk; it only ever grows
    if (d->r_work) (void)hipFree(d->r_work);
    d->r_work = nullptr;
    d->r_rows = 0;
    SVC_HIP(hipMalloc((void**)&d->r_work, RefineAreas<T>::bytes(d, cap_rows)));
    d->r_rows = cap_rows;
  }
  const RefineAreas<T> ra(d, ro ? d->r_rows : 0);
  d->kernel_ms = 0.0;
  d->launches = 0;
  for (int64_t r0 = 0; r0 < n_rows; r0 += cap_rows) {
    const int n = (int)std::min(cap_rows, n_rows - r0), n_pad = (n + TILE - 1) / TILE * TILE;
    if (const int rc = prepare_chunk<T>(d, a, host, dev, rows_dtype, ld, r0, n, n_pad, true)) return rc;      // decode always scales
    hipLaunchKernelGGL((k_decode_tiles<T>), dim3((unsigned)(n_pad / TILE), (unsigned)p.n_strips), dim3(256), 0, d->stream, a.conv, (const T*)d->table,
                       (int)d->Kp, n, (unsigned)d->S, (int)d->col_tiles, (int)p.tiles_per_strip, a.pval, a.pcol, (int)cap_rows);
    SVC_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_decode_finish<T>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, d->stream, a.pval, a.pcol, (int)cap_rows, (int)p.n_strips,
                       n, (const T*)a.conv, (const T*)d->table, (int)d->Kp, a.sims, a.best);
    SVC_HIP(hipGetLastError());
    if (ro) SVC_HIP(refine_chunk<T>(d, ra, (const T*)a.conv, a.best, n, ro->iterations));
    SVC_HIP(hipEventRecord(d->ev[1], d->stream));
    if (best) SVC_HIP(hipMemcpyAsync(best + r0, a.best, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream));
    if (sims) SVC_HIP(hipMemcpyAsync(sims + r0, a.sims, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
    if (ro) {
      SVC_HIP(hipMemcpyAsync(ro->x + (size_t)r0 * d->r_dim, ra.x, (size_t)n * d->r_dim * 8, hipMemcpyDeviceToHost, d->stream));
      if (ro->f) SVC_HIP(hipMemcpyAsync(ro->f + r0, ra.f, (size_t)n * 8, hipMemcpyDeviceToHost, d->stream));
      if (ro->status) SVC_HIP(hipMemcpyAsync(ro->status + r0, ra.status, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream));
    }
    SVC_HIP(hipStreamSynchronize(d->stream));
    if (const int rc = elapsed(d->ev[0], d->ev[1], &d->kernel_ms)) return rc;
    d->launches += ro ? 5 : 3;
  }
  return SSN_OK;
}

// The similarity map of ssn_decoder_map.  Rows as decode_rows takes them.  A device output is written in place by the kernel; a host
// output goes chunk by chunk through the device stage (dense, leading dimension S) and the pinned area, and from there row by row
// into `out`.  Rows per chunk: whole tiles that fit the row scratch (upload staging + converted rows) and, for a host output, the
// stage - never n_rows x S.  Column tiles are cut into runs as ssn_decoder::plan cuts strips (tiles_per_part), without the slot limit.
// Every tile is computed alone, so neither cut shows in the result.  Single-buffered: the copy back of a chunk is not
// overlapped with the next chunk's kernels.
template <typename T, typename TO>
int map_rows(ssn_decoder* d, const double* host, const void* dev, int rows_dtype, int64_t ld, int64_t n_rows, int flags, TO* out, bool out_on_device,
             int64_t out_ld) {
  DevGuard g(d->device);
  const int64_t S = d->S, t_tiles = (n_rows + TILE - 1) / TILE;
  int64_t cap = std::min<int64_t>(d->scratch_bytes / (TILE * d->row_bytes(0)), (1 << 24) / TILE);      // >= 1: min_scratch() is larger
  if (!out_on_device) {
    const int64_t want = d->m_stage_bytes ? d->m_stage_bytes : d->default_map_stage();
    if (want < d->min_map_stage(sizeof(TO)))
      return fail(SSN_EINVAL, "ssn_decoder_map: map stage of %lld bytes too small for one %d-row tile of %lld samples (%lld bytes)", (long long)want, TILE,
                  (long long)S, (long long)d->min_map_stage(sizeof(TO)));
    if (d->m_alloc != want) {
      d->drop_map_stage();
      SVC_HIP(hipMalloc((void**)&d->m_dev, (size_t)want));
      if (hipHostMalloc((void**)&d->m_pin, (size_t)want, hipHostMallocDefault) != hipSuccess) { d->drop_map_stage(); return fail(SSN_ENOMEM, "ssn_decoder_map: hipHostMalloc of %lld bytes", (long long)want); }
      d->m_alloc = want;
    }
    cap = std::min<int64_t>(cap, want / d->min_map_stage(sizeof(TO)));
  }
  const int64_t chunk_tiles = cut_rows(t_tiles, cap), cap_rows = chunk_tiles * TILE;
  const int64_t tpr = tiles_per_part(d->col_tiles, std::min<int64_t>(d->col_tiles, 4096), chunk_tiles, 2 * (int64_t)d->n_cu);      // nothing is kept per run
  const int64_t n_runs = (d->col_tiles + tpr - 1) / tpr;
  const Areas<T> a(d, cap_rows, 0);
  const bool scale = flags & SSN_MAP_NORMALIZE;
  const int square = flags & SSN_MAP_SQUARE ? 1 : 0;
  d->kernel_ms = 0.0;
  d->launches = 0;
  for (int64_t r0 = 0; r0 < n_rows; r0 += cap_rows) {
    const int n = (int)std::min(cap_rows, n_rows - r0), n_pad = (n + TILE - 1) / TILE * TILE;
    if (const int rc = prepare_chunk<T>(d, a, host, dev, rows_dtype, ld, r0, n, n_pad, scale)) return rc;
    TO* dst = out_on_device ? out + (size_t)r0 * out_ld : (TO*)d->m_dev;
    hipLaunchKernelGGL((k_decode_map<T, TO>), dim3((unsigned)(n_pad / TILE), (unsigned)n_runs), dim3(256), 0, d->stream, (const T*)a.conv, (const T*)d->table,
                       (int)d->Kp, n, (unsigned)S, (int)d->col_tiles, (int)tpr, square, dst, (long long)(out_on_device ? out_ld : S));
    SVC_HIP(hipGetLastError());
    SVC_HIP(hipEventRecord(d->ev[1], d->stream));
    if (!out_on_device) SVC_HIP(hipMemcpyAsync(d->m_pin, d->m_dev, (size_t)n * S * sizeof(TO), hipMemcpyDeviceToHost, d->stream));
    SVC_HIP(hipStreamSynchronize(d->stream));
    if (!out_on_device) {
      const TO* src = (const TO*)d->m_pin;
      if (out_ld == S) memcpy(out + (size_t)r0 * S, src, (size_t)n * S * sizeof(TO));
      else for (int64_t r = 0; r < n; ++r) memcpy(out + (size_t)(r0 + r) * out_ld, src + (size_t)r * S, (size_t)S * sizeof(TO));
    }
    if (const int rc = elapsed(d->ev[0], d->ev[1], &d->kernel_ms)) return rc;
    d->launches += 2;
  }
  return SSN_OK;
}

template <typename T>
int upload_refine(ssn_decoder* d,const double* dft, const double* M, const double* w, const double* points, const double* lo, const double* hi,
                  const double* pitch) {
  const int64_t K = d->r_K, Kp = d->Kp, width = d->K, dim = d->r_dim;
  std::vector<T> tab((size_t)2 * K * Kp, T(0)), m((size_t)K * dim);
  for (int64_t r = 0; r < 2 * K; ++r)
    for (int64_t c = 0; c < width; ++c) tab[(size_t)r * Kp + c] = (T)(w[r / 2] * dft[(size_t)r * width + c]);
  for (int64_t i = 0; i < K * dim; ++i) m[i] = (T)M[i];
  std::vector<double> box((size_t)3 * dim);
  for (int64_t a = 0; a < dim; ++a) { box[a] = lo[a]; box[dim + a] = hi[a]; box[2 * dim + a] = pitch[a]; }
  SVC_HIP(hipMalloc(&d->r_dft, tab.size() * sizeof(T)));
  SVC_HIP(hipMalloc(&d->r_M, m.size() * sizeof(T)));
  SVC_HIP(hipMalloc((void**)&d->r_points, (size_t)d->S * dim * 8));
  SVC_HIP(hipMalloc((void**)&d->r_box, box.size() * 8));
  SVC_HIP(hipMemcpy(d->r_dft, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice));
  SVC_HIP(hipMemcpy(d->r_M, m.data(), m.size() * sizeof(T), hipMemcpyHostToDevice));
  SVC_HIP(hipMemcpy(d->r_points, points, (size_t)d->S * dim * 8, hipMemcpyHostToDevice));
  SVC_HIP(hipMemcpy(d->r_box, box.data(), box.size() * 8, hipMemcpyHostToDevice));
  return SSN_OK;
}

// The composition the fused kernel replaces (tools/bench_decode.py, shape (c)): the parent's k_gemm_nt_mfma_f32 into an n_rows x S
// buffer of its own, then k_argmax_partial with one slice per row.
int decode_rows_composed(ssn_decoder* d, const double* host, int64_t n_rows, int32_t* best) {
  DevGuard g(d->device);
  const int64_t cap_rows = d->scratch_bytes / (TILE * d->row_bytes(0)) * TILE;
  if (n_rows > cap_rows) return fail(SSN_EINVAL, "ssn_decoder_rows_composed: %lld rows do not fit the scratch area in one chunk (%lld do)", (long long)n_rows, (long long)cap_rows);
  if ((double)n_rows * (double)d->S > (double)(1 << 29)) return fail(SSN_EINVAL, "ssn_decoder_rows_composed: a %lld x %lld similarity matrix is more than 2 GB", (long long)n_rows, (long long)d->S);
  const Areas<float> a(d, cap_rows, 0);
  const int n = (int)n_rows, n_pad = (n + TILE - 1) / TILE * TILE;
  float *C = nullptr, *part = nullptr;
  SVC_HIP(hipMalloc(&C, (size_t)n_rows * d->S * 4));
  if (hipMalloc(&part, (size_t)n_rows * 8) != hipSuccess) { (void)hipFree(C); return fail(SSN_ENOMEM, "hipMalloc"); }
  std::vector<int32_t> idx((size_t)n_rows);
  auto run = [&]() -> int {
    if (const int rc = prepare_chunk<float>(d, a, host, nullptr, 0, d->K, 0, n, n_pad, true)) return rc;      // host rows from row 0, scaled
    SVC_HIP(ssn::launch_gemm_nt<float>(d->stream, a.conv, (int)d->Kp, (const float*)d->table, (int)d->Kp, C, (int)d->S, n, (int)d->S, (int)d->Kp, 1));
    SVC_HIP(ssn::launch_argmax_partial<float>(d->stream, C, (long long)n_rows * d->S, part, n, 1));
    SVC_HIP(hipEventRecord(d->ev[1], d->stream));
    SVC_HIP(hipMemcpyAsync(idx.data(), part + n_rows, (size_t)n_rows * 4, hipMemcpyDeviceToHost, d->stream));
    SVC_HIP(hipStreamSynchronize(d->stream));
    d->kernel_ms = 0.0;
    if (const int rc = elapsed(d->ev[0], d->ev[1], &d->kernel_ms)) return rc;
    d->launches = 3;
    return SSN_OK;
  };
  const int rc = run();
  (void)hipFree(C);
  (void)hipFree(part);
  if (rc == SSN_OK) for (int64_t r = 0; r < n_rows; ++r) best[r] = (int32_t)((int64_t)idx[r] - r * d->S);      // slice r starts at r S
  return rc;
}

// the table made where it is used: a float64 encoder of its own writes every chunk of sample points into the padded table, in
// the decoder's dtype; the encoder and its scratch area go away before the decoder is handed out
int encode_table(ssn_decoder* d, const double* points, int64_t K, int32_t dim, const double* M, const double* w, int64_t enc_scratch_bytes) {
  const int64_t Sp = d->col_tiles * TILE;
  SVC_HIP(hipMalloc(&d->table, (size_t)Sp * d->Kp * d->esz));
  SVC_HIP(hipMemset(d->table, 0, (size_t)Sp * d->Kp * d->esz));
  ssn_encoder* enc = nullptr;
  int rc = ssn_encoder_create(SSN_F64, d->device, d->K, K, dim, M, w, enc_scratch_bytes, &enc);
  if (rc != SSN_OK) return rc;
  rc = ssn::encoder_encode_into(enc, points, d->S, d->table, d->dtype, d->Kp);
  ssn_encoder_destroy(enc);
  return rc;
}

// what ssn_decoder_create and ssn_decoder_create_from_points share: checks, stream, events and scratch; `fill` makes the table
template <typename Fill>
int create_decoder(const char* who, int32_t dtype, int32_t device, int64_t n_samples, int64_t width, int64_t scratch_bytes, ssn_decoder** out, Fill fill) {
  if (dtype != SSN_F32 && dtype != SSN_F64) return fail(SSN_EINVAL, "%s: unknown dtype %d", who, dtype);
  if (width <= 0 || width > (1 << 20)) return fail(SSN_EINVAL, "%s: width %lld outside 1 .. 2^20", who, (long long)width);
  if (n_samples <= 0 || n_samples > INT32_MAX)
    return fail(SSN_EINVAL, "%s: n_samples %lld outside 1 .. 2^31 - 1", who, (long long)n_samples);
  std::unique_ptr<ssn_decoder> d(new ssn_decoder);
  d->dtype = dtype;
  d->esz = dtype == SSN_F32 ? 4 : 8;
  d->S = n_samples;
  d->K = width;
  d->Kp = (width + KPAD - 1) / KPAD * KPAD;
  d->col_tiles = (n_samples + TILE - 1) / TILE;
  if (const int rc = d->open(who, device, scratch_bytes, d->min_scratch(), "%d-row tile of width %lld", TILE, (long long)width)) return rc;
  DevGuard g(device);
  hipDeviceProp_t prop;
  SVC_HIP(hipGetDeviceProperties(&prop, device));
  d->n_cu = std::max(1, prop.multiProcessorCount);
  const int rc = fill(d.get());
  if (rc != SSN_OK) return rc;
  *out = d.release();
  return SSN_OK;
}

}  // namespace

extern "C" {

int ssn_decoder_create(int32_t dtype, int32_t device, const double* table, int64_t n_samples, int64_t width, int64_t scratch_bytes,
                       ssn_decoder** out) {
  if (!out) return fail(SSN_EINVAL, "ssn_decoder_create: null handle");
  *out = nullptr;
  if (!table) return fail(SSN_EINVAL, "ssn_decoder_create: null table");
  return create_decoder("ssn_decoder_create", dtype, device, n_samples, width, scratch_bytes, out, [&](ssn_decoder* d) {
    return dtype == SSN_F32 ? upload_table<float>(d, table) : upload_table<double>(d, table);
  });
}

int ssn_decoder_create_from_points(int32_t dtype, int32_t device, const double* points, int64_t n_samples, int64_t width, int64_t K, int32_t dim,
                                   const double* M, const double* w, int64_t scratch_bytes, int64_t enc_scratch_bytes, ssn_decoder** out) {
  if (!out) return fail(SSN_EINVAL, "ssn_decoder_create_from_points: null handle");
  *out = nullptr;
  if (!points || !M || !w) return fail(SSN_EINVAL, "ssn_decoder_create_from_points: null argument");
  return create_decoder("ssn_decoder_create_from_points", dtype, device, n_samples, width, scratch_bytes, out, [&](ssn_decoder* d) {
    return encode_table(d, points, K, dim, M, w, enc_scratch_bytes);
  });
}

void ssn_decoder_destroy(ssn_decoder* dec) { delete dec; }

int ssn_decoder_rows(ssn_decoder* dec, const double* rows, int64_t n_rows, int32_t* best, double* sims) {
  if (!dec) return fail(SSN_EINVAL, "ssn_decoder_rows: null decoder");
  if (n_rows < 0) return fail(SSN_EINVAL, "ssn_decoder_rows: negative n_rows");
  if (n_rows == 0) return SSN_OK;
  if (!rows || !best) return fail(SSN_EINVAL, "ssn_decoder_rows: null argument");
  return dec->dtype == SSN_F32 ? decode_rows<float>(dec, rows, nullptr, 0, dec->K, n_rows, best, sims)
                               : decode_rows<double>(dec, rows, nullptr, 0, dec->K, n_rows, best, sims);
}

int ssn_decoder_rows_device(ssn_decoder* dec, const void* rows_dev, int32_t rows_dtype, int64_t ld, int64_t n_rows, int32_t* best, double* sims) {
  if (!dec) return fail(SSN_EINVAL, "ssn_decoder_rows_device: null decoder");
  if (n_rows < 0) return fail(SSN_EINVAL, "ssn_decoder_rows_device: negative n_rows");
  if (const int rc = check_rows("ssn_decoder_rows_device", "rows", rows_dtype, ld, dec->K)) return rc;
  if (n_rows == 0) return SSN_OK;
  if (!rows_dev || !best) return fail(SSN_EINVAL, "ssn_decoder_rows_device: null argument");
  return dec->dtype == SSN_F32 ? decode_rows<float>(dec, nullptr, rows_dev, rows_dtype, ld, n_rows, best, sims)
                               : decode_rows<double>(dec, nullptr, rows_dev, rows_dtype, ld, n_rows, best, sims);
}

int ssn_decoder_set_refine(ssn_decoder* dec, const double* dft, int64_t K, const double* M, const double* w, int32_t dim, const double* points,
                           const double* lo, const double* hi, const double* pitch) {
  if (!dec) return fail(SSN_EINVAL, "ssn_decoder_set_refine: null decoder");
  if (!dft || !M || !w || !points || !lo || !hi || !pitch) return fail(SSN_EINVAL, "ssn_decoder_set_refine: null argument");
  if (dim < 1 || dim > 3) return fail(SSN_EINVAL, "ssn_decoder_set_refine: dim %d is not supported: k_decode_refine exists for dim 1, 2 and 3", dim);
  if (K < 1 || K > dec->K) return fail(SSN_EINVAL, "ssn_decoder_set_refine: %lld bins outside 1 .. width %lld", (long long)K, (long long)dec->K);
  DevGuard g(dec->device);
  dec->drop_refine();
  dec->r_dim = dim;
  dec->r_K = K;
  const int rc = dec->dtype == SSN_F32 ? upload_refine<float>(dec, dft, M, w, points, lo, hi, pitch) : upload_refine<double>(dec, dft, M, w, points, lo, hi, pitch);
  if (rc != SSN_OK) dec->drop_refine();
  return rc;
}

static int refine_args(const char* who, ssn_decoder* dec, int64_t n_rows, int32_t iterations) {
  if (!dec) return fail(SSN_EINVAL, "%s: null decoder", who);
  if (n_rows < 0) return fail(SSN_EINVAL, "%s: negative n_rows", who);
  if (iterations < 0) return fail(SSN_EINVAL, "%s: negative iterations", who);
  if (!dec->r_dim) return fail(SSN_EINVAL, "%s: no refinement tables: call ssn_decoder_set_refine first", who);
  return SSN_OK;
}

int ssn_decoder_refine_rows(ssn_decoder* dec, const double* rows, int64_t n_rows, int32_t iterations, double* x, int32_t* best, double* f,
                            int32_t* status) {
  const int rc = refine_args("ssn_decoder_refine_rows", dec, n_rows, iterations);
  if (rc != SSN_OK || n_rows == 0) return rc;
  if (!rows || !x) return fail(SSN_EINVAL, "ssn_decoder_refine_rows: null argument");
  const RefineOut ro{iterations, x, f, status};
  return dec->dtype == SSN_F32 ? decode_rows<float>(dec, rows, nullptr, 0, dec->K, n_rows, best, nullptr, &ro)
                               : decode_rows<double>(dec, rows, nullptr, 0, dec->K, n_rows, best, nullptr, &ro);
}

int ssn_decoder_refine_rows_device(ssn_decoder* dec, const void* rows_dev, int32_t rows_dtype, int64_t ld, int64_t n_rows, int32_t iterations,
                                   double* x, int32_t* best, double* f, int32_t* status) {
  const int rc = refine_args("ssn_decoder_refine_rows_device", dec, n_rows, iterations);
  if (rc != SSN_OK) return rc;
  if (const int rc = check_rows("ssn_decoder_refine_rows_device", "rows", rows_dtype, ld, dec->K)) return rc;
  if (n_rows == 0) return SSN_OK;
  if (!rows_dev || !x) return fail(SSN_EINVAL, "ssn_decoder_refine_rows_device: null argument");
  const RefineOut ro{iterations, x, f, status};
  return dec->dtype == SSN_F32 ? decode_rows<float>(dec, nullptr, rows_dev, rows_dtype, ld, n_rows, best, nullptr, &ro)
                               : decode_rows<double>(dec, nullptr, rows_dev, rows_dtype, ld, n_rows, best, nullptr, &ro);
}

int ssn_decoder_rows_composed(ssn_decoder* dec, const double* rows, int64_t n_rows, int32_t* best) {
  if (!dec || !rows || !best || n_rows <= 0) return fail(SSN_EINVAL, "ssn_decoder_rows_composed: null or empty argument");
  if (dec->dtype != SSN_F32) return fail(SSN_EUNSUPPORTED, "ssn_decoder_rows_composed: f32 decoders only (k_gemm_nt_mfma_f32)");
  return decode_rows_composed(dec, rows, n_rows, best);
}

int ssn_decoder_map(ssn_decoder* dec, const void* rows, int32_t rows_on_device, int32_t rows_dtype, int64_t rows_ld, int64_t n_rows, int32_t flags,
                    void* out, int32_t out_on_device, int32_t out_dtype, int64_t out_ld) {
  if (!dec) return fail(SSN_EINVAL, "ssn_decoder_map: null decoder");
  if (n_rows < 0) return fail(SSN_EINVAL, "ssn_decoder_map: negative n_rows");
  if (flags & ~(SSN_MAP_NORMALIZE | SSN_MAP_SQUARE)) return fail(SSN_EINVAL, "ssn_decoder_map: unknown flags 0x%x", flags);
  if (rows_on_device)      // (host rows are dense doubles)
    if (const int rc = check_rows("ssn_decoder_map", "rows", rows_dtype, rows_ld, dec->K, " of the rows")) return rc;
  if (out_dtype != SSN_F32 && out_dtype != SSN_F64) return fail(SSN_EINVAL, "ssn_decoder_map: unknown out_dtype %d", out_dtype);
  if (out_dtype == SSN_F32 && dec->dtype == SSN_F64)
    return fail(SSN_EINVAL, "ssn_decoder_map: out_dtype f32 is narrower than the f64 decoder's (narrowing is not offered)");
  if (out_ld < dec->S) return fail(SSN_EINVAL, "ssn_decoder_map: leading dimension %lld of the output below n_samples %lld", (long long)out_ld, (long long)dec->S);
  if (n_rows == 0) return SSN_OK;
  if (!rows || !out) return fail(SSN_EINVAL, "ssn_decoder_map: null argument");
  const double* host = rows_on_device ? nullptr : (const double*)rows;
  const void* dev = rows_on_device ? rows : nullptr;
  const int64_t ld = rows_on_device ? rows_ld : dec->K;
  if (dec->dtype == SSN_F64) return map_rows<double, double>(dec, host, dev, rows_dtype, ld, n_rows, flags, (double*)out, out_on_device != 0, out_ld);
  return out_dtype == SSN_F32 ? map_rows<float, float>(dec, host, dev, rows_dtype, ld, n_rows, flags, (float*)out, out_on_device != 0, out_ld)
                              : map_rows<float, double>(dec, host, dev, rows_dtype, ld, n_rows, flags, (double*)out, out_on_device != 0, out_ld);
}

int ssn_decoder_set_map_stage(ssn_decoder* dec, int64_t bytes) {
  if (!dec) return fail(SSN_EINVAL, "ssn_decoder_set_map_stage: null decoder");
  if (bytes < 0) return fail(SSN_EINVAL, "ssn_decoder_set_map_stage: negative size");
  if (bytes && bytes < dec->min_map_stage(dec->esz))
    return fail(SSN_EINVAL, "ssn_decoder_set_map_stage: %lld bytes too small for one %d-row tile of %lld samples (%lld bytes)", (long long)bytes, TILE,
                (long long)dec->S, (long long)dec->min_map_stage(dec->esz));
  dec->m_stage_bytes = bytes;      // the areas are made again, at this size, by the next host-output map
  return SSN_OK;
}

int ssn_decoder_get_info(ssn_decoder* dec, int64_t n_rows, ssn_decoder_info* out) {
  if (!dec || !out || n_rows < 0) return fail(SSN_EINVAL, "ssn_decoder_get_info: null argument");
  const Plan p = dec->plan(n_rows);
  out->row_chunk = p.chunk_tiles * TILE;
  out->n_chunks = n_rows ? p.n_chunks : 0;
  out->n_strips = p.n_strips;
  out->tiles_per_strip = p.tiles_per_strip;
  out->tile = TILE;
  out->scratch_bytes = dec->scratch_bytes;
  out->min_scratch_bytes = dec->min_scratch();
  out->slot_bytes = TILE * (int64_t)(dec->esz + 4);
  out->padded_width = dec->Kp;
  out->last_launches = dec->launches;
  out->last_kernel_ms = dec->kernel_ms;
  return SSN_OK;
}

}  // extern "C"
