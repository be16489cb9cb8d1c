// ssn_micro.hpp - what every glue micro-operator (ssn::MicroKind) computes, stated once.
//
// Four kernels run micro-operators and each walks memory its own way: k_program (one workgroup of 1024 threads, the whole
// operator), k_vecops (a grid-stride loop), k_round's glue_body (one chunk per block) and the time-batched stages
// (kb_elementwise_at: one element of one block row).  The meaning of a kind does not depend on the walk, so it lives here and
// the kernels bring the walk:
//
//   micro_elementwise   M_FILL, M_AXPY_INC, M_AXPY_SET, M_LOWPASS, M_TABLE, M_ROW_IN, M_ROW_OUT, M_PROBE: resolves the base
//                       pointers and whatever depends on the timestep, then hands a (load(i), store(i, v)) pair to the caller's
//                       walker.  A walker is an object with
//                         walk(len, load, store)   store(i, load(i)) for the elements i < len that this thread owns
//                         walk.overflow()          a probe sample found no slot: the one thread that reports it sets the flag
//                         walk.step()              timesteps completed before the one being executed.  A call, not an argument:
//                                                  the round kernel reads the counter from memory, and read inside the case that
//                                                  needs it the load is issued beside the descriptor's; read up front it was one
//                                                  more dependent trip to memory in front of every hand-off, table row and probe
//   micro_lincomb       M_LINCOMB for U elements of one thread (the term loop is outermost over the U accumulators)
//   micro_rows          M_MATVEC_INC/SET, M_ENS_FINISH, M_REDUCE_SET/INC (micro_row_kind): one output row per call of the body
//                       that goes to  walk.rows(len, row)   row(r) for the rows r < len that this thread owns
//   micro_gate, micro_argmax_gather   M_GATE, M_ARGMAX_GATHER: one workgroup of NT threads, the whole vector
//
// Nothing here owns workgroup memory (the round kernel sizes one dynamic allocation for its hungriest body; a static array in
// a shared function would be added to every block): the whole-vector kinds take the caller's.  Everything is force-inlined
// into its caller and reads the descriptor's uniform fields in place.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "ssn_launch.hpp"

namespace ssn {

template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Element-wise kinds.  Op: MicroOp<T> (dbase = xbase = the signal vector) or
// BatchOp<T> (dbase / xbase = the block-buffer rows written / read; no row hand-offs there).  ctx is read for block_start only.
template <typename T, typename Op, typename W>
__device__ __forceinline__ void micro_elementwise(const Op& op, T* dbase, const T* xbase, const StepCtx* ctx, W&& walk) {
  constexpr bool STEP_OP = std::is_same<Op, MicroOp<T>>::value;
  switch (op.kind) {
    case M_FILL:
      { T* const d = dbase + op.dst; walk(op.len, [&](auto) { return op.a; }, [&](auto i, T v) { d[i] = v; }); }
      break;
    case M_AXPY_INC:
      { T* const d = dbase + op.dst; const T* const x = xbase + op.src;
        walk(op.len, [&](auto i) { return d[i] + op.a * x[i]; }, [&](auto i, T v) { d[i] = v; }); }
      break;
    case M_AXPY_SET:
      { T* const d = dbase + op.dst; const T* const x = xbase + op.src;
        walk(op.len, [&](auto i) { return op.a * x[i]; }, [&](auto i, T v) { d[i] = v; }); }
      break;
    case M_LOWPASS:   // dst = a*dst + b*src, b = (1-a)*gain
      { T* const d = dbase + op.dst; const T* const x = xbase + op.src;
        walk(op.len, [&](auto i) { return op.a * d[i] + op.b * x[i]; }, [&](auto i, T v) { d[i] = v; }); }
      break;
    case M_TABLE: {   // p0 = TableSlot*: the row the table's index list names for this step, zeros outside the list
      const TableSlot* t = (const TableSlot*)op.p0;
      const long long rel = walk.step() - t->first_step;
      int row = -1;
      if (rel >= 0 && rel < t->n_idx) row = t->idx[rel];
      const bool have = row >= 0 && row < t->n_rows;
      const T* const trow = (const T*)t->rows + (have ? (size_t)row * t->width : 0);
      T* const d = dbase + op.dst;
      walk(op.len, [&](auto i) { return have ? trow[i] : T(0); }, [&](auto i, T v) { d[i] = v; });
      break;
    }
    case M_PROBE: {   // p0 = ProbeSlot*; src, len = width: every `every`-th step's values (a batched stage samples the row it wrote)
      const ProbeSlot* ps = (const ProbeSlot*)op.p0;
      const long long s1 = walk.step() + 1;
      if (s1 % ps->every == 0) {
        const long long slot = s1 / ps->every - 1 - ps->base_slot;
        if (slot >= 0 && slot < ps->capacity) {
          T* const out = (T*)ps->data + (size_t)slot * op.len;
          const T* const x = dbase + op.src;
          walk(op.len, [&](auto i) { return x[i]; }, [&](auto i, T v) { out[i] = v; });
        } else {
          walk.overflow();
        }
      }
      break;
    }
    // hand-offs between the signal vector and the block buffer p0 ([rows][i0 = n_sig], i1 = offset in a row): the row of this
    // step is step - block_start + 1
    case M_ROW_IN:    // sig[dst..] = bsig[row][i1..]
      if constexpr (STEP_OP) {
        const T* const x = (const T*)op.p0 + (size_t)(walk.step() - ctx->block_start + 1) * op.i0 + op.i1;
        T* const d = dbase + op.dst;
        walk(op.len, [&](auto i) { return x[i]; }, [&](auto i, T v) { d[i] = v; });
      }
      break;
    case M_ROW_OUT:   // bsig[row][i1..] = sig[src..]
      if constexpr (STEP_OP) {
        T* const d = (T*)op.p0 + (size_t)(walk.step() - ctx->block_start + 1) * op.i0 + op.i1;
        const T* const x = xbase + op.src;
        walk(op.len, [&](auto i) { return x[i]; }, [&](auto i, T v) { d[i] = v; });
      }
      break;
    default:
      break;
  }
}

// M_LINCOMB: dst = a * dst + b * (c + sum_k alpha_k * sig[src_k + i]) for the elements i = first + u * stride < len, u < U;
// p0 = LinTerm[i0].  Per element: acc = c, acc += alpha_k * x_k[i] in term order; a == 0 does not read dst.
template <typename T, int U, typename I>
__device__ __forceinline__ void micro_lincomb(const MicroOp<T>& op, T* sig, const I first, const I stride) {
  const LinTerm<T>* const t = (const LinTerm<T>*)op.p0;
  const int nt = (int)op.i0;
  T* const d = sig + op.dst;
  T acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = op.c;
  for (int k = 0; k < nt; ++k) {
    const T alpha = t[k].alpha;
    const T* const x = sig + t[k].src;
#pragma unroll
    for (int u = 0; u < U; ++u) { const I i = first + u * stride; if (i < op.len) acc[u] += alpha * x[i]; }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const I i = first + u * stride;
    if (i < op.len) d[i] = (op.a != T(0) ? op.a * d[i] : T(0)) + op.b * acc[u];
  }
}

// Row kinds (micro_row_kind): one output row r < len per call of the body that the caller's walker gets - walk.rows(len, row)
// calls row(r) for the rows this thread owns.  Sums run in a fixed order, independent reads are issued together.
template <typename T, typename W>
__device__ __forceinline__ void micro_rows(const MicroOp<T>& op, T* sig, W&& walk) {
  switch (op.kind) {
    case M_MATVEC_INC:
    case M_MATVEC_SET: {   // p0 = W (rows x ld), i0 = cols, i1 = ld; len = rows
      const T* Wm = (const T*)op.p0;
      walk.rows(op.len, [&](const long long r) {
        T s = T(0);
        for (int c = 0; c < (int)op.i0; ++c) s += Wm[(size_t)r * op.i1 + c] * sig[op.src + c];
        if (op.kind == M_MATVEC_INC) sig[op.dst + r] += s; else sig[op.dst + r] = s;
      });
      break;
    }
    case M_ENS_FINISH: {   // p0 = partials [K][P][dout], p1 = dst_idx int32 [K*dout]; len = K*dout, i0 = P, i1 = dout
      const T* part = (const T*)op.p0;
      // src > 0: the array keeps two sets of partial sums, src elements apart, by timestep parity (round plan).  The item plan
      // leaves src = 0 (plan(): `MOp f{}` where it pushes M_ENS_FINISH), so k_program never takes this branch.
      if (op.src > 0) part += (size_t)(walk.step() & 1) * (size_t)op.src;
      const int* didx = (const int*)op.p1;
      const int P = (int)op.i0, dout = (int)op.i1;
      walk.rows(op.len, [&](const long long i) {
        const long long k = i / dout, r = i - k * dout;
        const int dst = didx[i];                 // (fetched beside the partial sums, not behind them)
        T s = T(0);
        int p = 0;
        for (; p + 8 <= P; p += 8) {             // eight partial sums in flight, added in workgroup order
          T v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = part[((size_t)k * P + p + q) * dout + r];
#pragma unroll
          for (int q = 0; q < 8; ++q) s += v[q];
        }
        {
          T v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = p + q < P ? part[((size_t)k * P + p + q) * dout + r] : T(0);
#pragma unroll
          for (int q = 0; q < 8; ++q) if (p + q < P) s += v[q];
        }
        sig[dst] = s;
      });
      break;
    }
    case M_REDUCE_SET:
    case M_REDUCE_INC: {   // p0 = partial [i0 chunks][i1 rows_pad]: dst[r] (+)= sum_c partial[c][r], in chunk order
      const T* part = (const T*)op.p0;
      const int nc = (int)op.i0;
      walk.rows(op.len, [&](const long long r) {
        T s = T(0);
        int c = 0;
        for (; c + 16 <= nc; c += 16) {          // sixteen chunk reads in flight (a reduction is one of the dependent trips of every
          T v[16];                               // population hop: 40 chunks are three trips this way, five with eight)
#pragma unroll
          for (int q = 0; q < 16; ++q) v[q] = part[(size_t)(c + q) * op.i1 + r];
#pragma unroll
          for (int q = 0; q < 16; ++q) s += v[q];
        }
        for (; c + 8 <= nc; c += 8) {
          T v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = part[(size_t)(c + q) * op.i1 + r];
#pragma unroll
          for (int q = 0; q < 8; ++q) s += v[q];
        }
        for (; c < nc; ++c) s += part[(size_t)c * op.i1 + r];
        if (op.kind == M_REDUCE_INC) sig[op.dst + r] += s; else sig[op.dst + r] = s;
      });
      break;
    }
    default:
      break;
  }
}

// The whole-vector kinds: one workgroup of NT threads; smem holds NT / 64 values of T, then as many int.

// M_GATE (reference slam.py:236-257's loop-closure correction): dst = open ? rate * (est - cur) : 0, open when the two
// d-vectors agree (dot product above the threshold) and the flag input is 0.  src = [est(d), cur(d), flag], len = d,
// a = threshold, b = rate.  The waves' sums are added left to right: NT is part of the result's rounding.
template <typename T, int NT>
__device__ __forceinline__ void micro_gate(const MicroOp<T>& op, T* __restrict__ sig, unsigned char* smem) {
  T* sred = reinterpret_cast<T*>(smem);
  const int tid = threadIdx.x;
  T part = T(0);
  for (long long i = tid; i < op.len; i += NT) part += sig[op.src + i] * sig[op.src + op.len + i];
  part = wave_sum(part);
  if ((tid & 63) == 0) sred[tid >> 6] = part;
  __syncthreads();
  T dot = sred[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) dot += sred[w];
  const T flag = sig[op.src + 2 * op.len];
  const bool open = (flag <= T(1e-3) && flag >= T(-1e-3)) && dot > op.a;
  for (long long i = tid; i < op.len; i += NT)
    sig[op.dst + i] = open ? op.b * (sig[op.src + i] - sig[op.src + op.len + i]) : T(0);
}

// M_ARGMAX_GATHER, the clean-up memory: dst = table[first argmax of sims].  p1 = sims (i0 rows, scratch), p0 = table
// (i0 x ld = i1), len = cols.  src = P > 0: p1 holds the first maxima of P consecutive slices (k_argmax_partial): P values,
// then their P row indices.  CU candidate reads in flight per thread; the row is copied by the caller's walker.
template <typename T, int NT, int CU, typename W>
__device__ __forceinline__ void micro_argmax_gather(const MicroOp<T>& op, T* __restrict__ sig, unsigned char* smem, W&& walk) {
  constexpr int NW = NT / 64;
  T* sred = reinterpret_cast<T*>(smem);
  int* sidx = reinterpret_cast<int*>(smem + NW * sizeof(T));
  const int tid = threadIdx.x;
  T best = T(-INFINITY);
  int bi = 0x7fffffff;
  const T* sims = (const T*)op.p1;
  const int n_cand = op.src > 0 ? (int)op.src : (int)op.i0;
  const int* cand_idx = op.src > 0 ? (const int*)(sims + op.src) : nullptr;
  for (int i0 = tid; i0 < n_cand; i0 += CU * NT) {       // examined in ascending order
    T v[CU];
    int vi[CU];
#pragma unroll
    for (int u = 0; u < CU; ++u) {
      const int i = i0 + u * NT;
      v[u] = i < n_cand ? sims[i] : T(-INFINITY);
      vi[u] = (cand_idx && i < n_cand) ? cand_idx[i] : i;
    }
#pragma unroll
    for (int u = 0; u < CU; ++u)
      if (v[u] > best) { best = v[u]; bi = vi[u]; }     // first maximum within a thread (ascending i)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T ov = __shfl_down(best, off, 64);
    const int oi = __shfl_down(bi, off, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { sred[tid >> 6] = best; sidx[tid >> 6] = bi; }
  __syncthreads();
  best = sred[0]; bi = sidx[0];
  for (int w = 1; w < NW; ++w)
    if (sred[w] > best || (sred[w] == best && sidx[w] < bi)) { best = sred[w]; bi = sidx[w]; }
  if (bi == 0x7fffffff) bi = 0;
  const T* const trow = (const T*)op.p0 + (size_t)bi * op.i1;
  T* const d = sig + op.dst;
  walk(op.len, [&](auto i) { return trow[i]; }, [&](auto i, T v) { d[i] = v; });
}

}  // namespace ssn
