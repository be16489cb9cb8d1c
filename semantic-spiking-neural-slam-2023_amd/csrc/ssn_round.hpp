// ssn_round.hpp - k_round: every mutually independent operator of a timestep in ONE launch.
//
// A SLAM timestep is a chain of ~25 dependency levels (reference networks/slam.py:259-307 wires ensembles, products
// and memories through un-filtered connections, so most of a step is sequential), and each level holds a few big
// operators next to a dozen 1 000 - 2 000 element vector operators.  A launch costs ~5 us on this GPU whatever it
// does, so one launch per operator (or per operator kind) makes the step launch-bound.  k_round runs a whole level:
// the host planner (ssn_host.hip, plan_rounds) assigns every operator of the step the earliest round its data
// hazards allow; a round's operators become the entries of ONE grid - entry i owns virtual blocks
// [first, first + gx * gy) - and each 256-thread workgroup runs the body its block belongs to:
//
//   RK_GLUE     one chunk (GLUE_CHUNK elements / GLUE_ROWS reduction rows) of one micro-operator: fill, axpy, lowpass,
//               table row, block-row hand-off, probe sample, partial-sum reductions, step counter.  The single-workgroup
//               interpreter k_program runs these back to back (~0.4 us each, latency-bound); here they run side by side.
//               What a kind computes is written once, in ssn_micro.hpp, for k_program, k_vecops, the time-batched stages and
//               this kernel alike: glue_body below only supplies the walk over one chunk (GlueWalk).
//   RK_GATE, RK_ARGMAX   whole-vector micro-operators (a dot product / an argmax decide what is written): one block;
//               micro_gate / micro_argmax_gather of ssn_micro.hpp at 256 threads
//   RK_MATVEC_*, RK_SPMV, RK_NEURONS, RK_DFT, RK_PES, RK_VOJA   the bodies of the stand-alone kernels (ssn_kernels.hpp)
//   RK_ENS_*    k_ensarray's body for the variants a SLAM network uses: the path integrator's oscillators (3 inputs, 4 or 5
//               decoded rows, spike-sparse decoders) and the product ensembles of the circular convolutions (1-D)
//
// Workgroup memory is one dynamic allocation sized for the round's hungriest body (no static LDS in any body: static
// allocations of all bodies would add up).
#pragma once
#include "ssn_kernels.hpp"

namespace ssn {

// The walks of a 256-thread block (ssn_micro.hpp brings what the operators compute).  GlueWalk, one chunk of an operator:
// U elements per thread from chunk * 256 U, loads before stores, or row chunk * GLUE_ROWS + tid; chunk 0 reports a probe overflow.
template <typename T, int U>
struct GlueWalk {
  int chunk, tid, sub;
  StepCtx* ctx;
  template <typename L, typename S>
  __device__ void operator()(long long len, L load, S store) const {
    const long long base = (long long)chunk * (U * 256);
    T v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const long long i = base + u * 256 + tid; if (i < len) v[u] = load(i); }
#pragma unroll
    for (int u = 0; u < U; ++u) { const long long i = base + u * 256 + tid; if (i < len) store(i, v[u]); }
  }
  template <typename R>
  __device__ void rows(long long len, R row) const { const long long r = (long long)chunk * GLUE_ROWS + tid; if (r < len) row(r); }
  __device__ void overflow() const { if (tid == 0 && chunk == 0) ctx->probe_overflow = 1; }
  __device__ long long step() const { return ctx->step + sub; }
};
// the whole vector, one element per thread and trip (the row copy of the argmax)
struct BlockWalk {
  template <typename L, typename S>
  __device__ void operator()(long long len, L load, S store) const { for (long long i = threadIdx.x; i < len; i += 256) store(i, load(i)); }
};

// One chunk of one micro-operator.  Element-wise kinds: elements [chunk * GLUE_CHUNK, ...) - four per thread; row kinds
// (micro_row_kind: reductions, ensemble finish, small matvec): rows [chunk * GLUE_ROWS, ...), one per thread.
template <typename T, bool ROWS = false>
__device__ __forceinline__ void glue_body(const MicroOp<T>& op, const int chunk, const int sub, T* sig, StepCtx* __restrict__ ctx) {
  // sub: timestep offset of this instance inside a pipelined launch sequence (the clock advances once per sequence)
  // ROWS: member of a chain - element-wise kinds handle element chunk * GLUE_ROWS + tid only, like the row kinds
  const int tid = threadIdx.x;
  constexpr int U = ROWS ? 1 : 4;
  static_assert(GLUE_CHUNK == 4 * 256 && GLUE_ROWS == 256, "a thread takes four elements of a chunk, or one of a chain's");
  const GlueWalk<T, U> walk{chunk, tid, sub, ctx};
  if (micro_row_kind(op.kind)) {
    micro_rows<T>(op, sig, walk);
  } else if (op.kind == M_LINCOMB) {
    micro_lincomb<T, U>(op, sig, (long long)chunk * (U * 256) + tid, (long long)256);
  } else if (op.kind == M_STEP_END) {
    if (tid == 0 && chunk == 0) ctx->step = ctx->step + 1;
  } else {
    micro_elementwise<T>(op, sig, sig, ctx, walk);
  }
}

// A serial chain (RK_SOLO): single-workgroup units in program order, a workgroup barrier between them.  At most one transform
// per chain, and it runs OUTSIDE the member loops (table: {n, code_0, sub_0, ...}; code < 0: the transform): inside a loop its
// descriptor and addressing stay live around the back edge and cost every block of the round kernel ~20 VGPRs.
template <typename T>
__device__ __forceinline__ void solo_body(const RoundArgs<T>& ra, const int* __restrict__ ch, unsigned char* smem) {
  // The chain table and the members' descriptors go to LDS first, all loads in flight together: read one at a time behind the
  // barrier of the member before, each member would start with two dependent trips to memory (table entry -> descriptor)
  // before the first load of its data - measured ~4 us per member instead of ~2.
  __shared__ int s_tab[2 * SOLO_MAX_MEMBERS + 2];
  __shared__ __align__(16) unsigned char s_ops[SOLO_MAX_MEMBERS * sizeof(MicroOp<T>)];
  const int tid = threadIdx.x;
  const int n = __builtin_amdgcn_readfirstlane(min(ch[0], SOLO_MAX_MEMBERS));
  if (tid < 2 * n) s_tab[tid] = ch[1 + tid];
  {
    constexpr int DW = (int)(sizeof(MicroOp<T>) / 4);
    static_assert(sizeof(MicroOp<T>) % 4 == 0, "descriptor copied by dwords");
    for (int i = tid; i < n * DW; i += 256) {
      const int q = i / DW, w = i - q * DW;
      const int code = ch[1 + 2 * q];
      if (code >= 0) reinterpret_cast<int*>(s_ops)[i] = reinterpret_cast<const int*>(ra.mops + code)[w];
    }
  }
  __syncthreads();
  auto members = [&](int q0, int q1) {
#pragma unroll 1
    for (int q = q0; q < q1; ++q) {
      const int sub = __builtin_amdgcn_readfirstlane(s_tab[2 * q + 1]);
      if (q) __syncthreads();
      const MicroOp<T>& op = reinterpret_cast<const MicroOp<T>*>(s_ops)[q];
      if (op.kind == M_GATE) micro_gate<T, 256>(op, ra.sig, smem);
      else if (op.kind == M_ARGMAX_GATHER) micro_argmax_gather<T, 256, 8>(op, ra.sig, smem, BlockWalk{});
      else {
        const bool rows = micro_row_kind(op.kind);
        const int chunks = (int)((op.len + (rows ? GLUE_ROWS : GLUE_CHUNK) - 1) / (rows ? GLUE_ROWS : GLUE_CHUNK));
#pragma unroll 1
        for (int c = 0; c < chunks; ++c) glue_body<T>(op, c, sub, ra.sig, ra.ctx);
      }
    }
  };
  int qd = n;                     // position of the transform (n: none)
#pragma unroll 1
  for (int q = 0; q < n; ++q) if (s_tab[2 * q] < 0) qd = q;
  qd = __builtin_amdgcn_readfirstlane(qd);
  members(0, qd);
  if (qd < n) {
    if (qd) __syncthreads();
    // (the descriptor is read through the constant address space: behind the stores of the members before it the compiler
    //  would otherwise fetch its uniform fields with vector loads and hold them in VGPRs)
    typedef const __attribute__((address_space(4))) DftArgs DftArgsK;
    if constexpr (sizeof(T) == 4) dft_body<true, DftArgsK>(*(DftArgsK*)(uintptr_t)(ra.arena + (size_t)(-s_tab[2 * qd] - 1) * 16), smem);
    members(qd + 1, n);
  }
}

// One virtual block of a round.
template <typename T>
__device__ __forceinline__ void round_block(const RoundArgs<T>& ra, int vb, unsigned char* smem) {
  int ei = 0;
  for (int q = 1; q < ra.n; ++q) if (vb >= ra.e[q].first) ei = q;       // (entries in ascending `first` order; uniform)
  const RoundEntry e = ra.e[ei];
  vb -= e.first;
  const int g = vb + e.lo;                   // (an operator may run in pieces, one per round: blocks [lo, lo + cnt) here)
  const int bx = g % e.gx, by = g / e.gx;
  switch (e.kind) {
    case RK_GLUE: {
      const GlueBlock gb = ((const GlueBlock*)e.args)[vb];
      if (gb.op >= 0) {
        glue_body<T>(ra.mops[gb.op], gb.chunk & 0xffffff, gb.chunk >> 24, ra.sig, ra.ctx);
      } else {
        const int* ch = ra.chain + (-gb.op - 1);
        const int n = ch[0];
        for (int q = 0; q < n; ++q) glue_body<T, true>(ra.mops[ch[1 + 2 * q]], gb.chunk, ch[2 + 2 * q], ra.sig, ra.ctx);
      }
      break;
    }
    case RK_SOLO: solo_body<T>(ra, (const int*)e.args, smem); break;
    case RK_GATE: micro_gate<T, 256>(*(const MicroOp<T>*)e.args, ra.sig, smem); break;
    case RK_ARGMAX: micro_argmax_gather<T, 256, 8>(*(const MicroOp<T>*)e.args, ra.sig, smem, BlockWalk{}); break;
    case RK_MATVEC_R1: matvec_body<T, true, 1, 4>(*(const MatvecArgs<T>*)e.args, bx, smem); break;
    // (one copy of the 16-rows-per-workgroup product for both: a plain product's descriptor has nr.V == nullptr)
    case RK_MATVEC_R4: case RK_MATVEC_NEURONS: matvec_neurons_body<T>(*(const MatvecNeuronsArgs<T>*)e.args, bx, smem); break;
    case RK_SPMV: spmv_body<T>(*(const SpmvArgs<T>*)e.args, bx, by, smem); break;
    case RK_NEURONS: neurons_body<T>(*(const NeuronsArgs<T>*)e.args, bx, smem); break;
    case RK_DFT:
      if constexpr (sizeof(T) == 4) dft_body<true>(*(const DftArgs*)e.args, smem);
      break;
    case RK_ENS_3_4_S: ens_body<T, 3, 4, 1, true>(*(const EnsArgs<T>*)e.args, bx, smem); break;
    case RK_ENS_3_5_S: ens_body<T, 3, 5, 1, true>(*(const EnsArgs<T>*)e.args, bx, smem); break;
    case RK_ENS_1_1_D: ens_body<T, 1, 1, 2, true>(*(const EnsArgs<T>*)e.args, bx, smem); break;
    case RK_ENS_SMALL: ens_small_body<T>(*(const EnsArgs<T>*)e.args, bx); break;
    case RK_GRID_LHS: grid_lhs_body<T>(*(const GridLhsArgs<T>*)e.args, bx); break;
    case RK_GRID_DOT: {      // row block bx of the remaining-axis factors against left-operand row by: similarities [by * nn + 16 bx ...)
      const GridDotArgs<T> g = *(const GridDotArgs<T>*)e.args;
      const MatvecArgs<T> m{g.W, g.A + (size_t)by * g.lda, g.dst + (size_t)by * g.nn, g.nn, g.k2, g.ldw, 1};
      matvec_body<T, true, 4>(m, bx, smem);
      break;
    }
    case RK_PES: pes_body<T>(*(const PesArgs<T>*)e.args, bx, by); break;
    case RK_VOJA: voja_body<T>(*(const VojaArgs<T>*)e.args, bx); break;
    default: break;
  }
}

#ifdef SSN_ROUND_STAMPS
// diagnostic build only (make F32_EXTRA=-DSSN_ROUND_STAMPS, tools/round_stamps.py): every block of every k_round launch leaves
// {launch id (RoundArgs::pad) << 32 | body kind << 24 | block index, s_memrealtime at its start, at its end} (100 MHz ticks)
constexpr unsigned int ROUND_STAMP_CAP = 1u << 20;
__device__ unsigned long long g_round_stamps[ROUND_STAMP_CAP][3];
__device__ unsigned int g_round_stamp_n;
inline long long read_round_stamps(unsigned long long* out, long long cap, int reset) {
  unsigned int n = 0;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_round_stamp_n), sizeof n) != hipSuccess) return -1;
  const long long m = std::min<long long>(std::min<long long>(n, ROUND_STAMP_CAP), cap);
  if (out && m > 0 && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_round_stamps), (size_t)m * 24) != hipSuccess) return -1;
  if (reset) { n = 0; if (hipMemcpyToSymbol(HIP_SYMBOL(g_round_stamp_n), &n, sizeof n) != hipSuccess) return -1; }
  return m;
}
#endif

// (experiment switch: -DSSN_ROUND_WAVES=8 asks the compiler for 64 VGPRs - 8 workgroups per CU instead of 7 - at the price of spills)
#ifdef SSN_ROUND_WAVES
#define SSN_ROUND_ATTR __attribute__((amdgpu_waves_per_eu(SSN_ROUND_WAVES, SSN_ROUND_WAVES)))
#else
#define SSN_ROUND_ATTR
#endif
template <typename T>
__global__ __launch_bounds__(256) SSN_ROUND_ATTR void k_round(RoundArgs<T> ra) {
  extern __shared__ __align__(16) unsigned char ssn_round_smem[];
  int vb = (int)blockIdx.x;
  if (ra.stride > 1u && vb >= ra.head) {
    const unsigned int m = gridDim.x - (unsigned int)ra.head;
    vb = ra.head + (int)(((unsigned long long)(unsigned int)(vb - ra.head) * ra.stride) % m);
  }
#ifdef SSN_ROUND_STAMPS
  unsigned long long st0, st1;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st0) :: "memory");
#endif
  // The latency-bound bodies at the head of the grid (transforms, serial chains, gate, argmax, glue: one workgroup each, and the
  // round lasts as long as the slowest of them) share their SIMDs with up to six waves of bandwidth-bound blocks: per-block
  // stamps (tools/round_stamps.py) show a transform that takes 9.5 us alone taking 25 - 50 us there.  Their waves issue first.
  if (vb < ra.prio) __builtin_amdgcn_s_setprio(3);
  round_block<T>(ra, vb, ssn_round_smem);
#ifdef SSN_ROUND_STAMPS
  if constexpr (sizeof(T) == 4) {
    __syncthreads();
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st1) :: "memory");
    if (threadIdx.x == 0) {
      int ei = 0;
      for (int q = 1; q < ra.n; ++q) if (vb >= ra.e[q].first) ei = q;
      const unsigned int i = atomicAdd(&g_round_stamp_n, 1u);
      if (i < ROUND_STAMP_CAP) {
        g_round_stamps[i][0] = ((unsigned long long)(unsigned int)ra.pad << 32) | ((unsigned long long)(ra.e[ei].kind & 255) << 24) | (unsigned long long)(blockIdx.x & 0xffffff);
        g_round_stamps[i][1] = st0;
        g_round_stamps[i][2] = st1;
      }
    }
  }
#endif
}

// (A persistent variant - all rounds of a step graph in one resident grid with grid barriers - was built, tested and
//  measured in round 2: 411 us per timestep against 142 us with one launch per round at SLAM config 3, because every
//  workgroup's release / acquire fence is a write-back + invalidate of its XCD's whole L2; the barrier measurements are
//  in tools/grid_barrier.hip and profiles/round2_grid_barrier.txt.  It was removed.)

template <typename T>
hipError_t launch_round(hipStream_t s, const RoundArgs<T>& ra, int n_blocks, size_t lds_bytes) {
  static std::atomic<uint64_t> configured{0};
  if (hipError_t e = set_max_dynamic_lds_once(reinterpret_cast<const void*>(&k_round<T>), 64 * 1024, configured); e != hipSuccess) return e;
  if (lds_bytes > 64 * 1024 || n_blocks <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_round<T>), dim3((unsigned)n_blocks), dim3(256), std::max<size_t>(lds_bytes, 64), s, ra);
  return hipGetLastError();
}

}  // namespace ssn
