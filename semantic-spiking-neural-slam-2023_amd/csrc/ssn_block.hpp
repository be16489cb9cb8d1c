// ssn_block.hpp - k_ens_block: a recurrent ensemble array stepped through a whole time block in ONE launch.
//
// Applies when the per-timestep core is an array of K ensembles whose only recurrence is
// ensemble k -> Lowpass -> ensemble k (the path integrator's VCO array, reference
// sspslam/networks/pathintegration.py:150-164): the K oscillators are then independent of each other
// inside a block - everything else they read (the velocity terms) was produced for all B timesteps of
// the block by the time-batched pre stage.  So instead of streaming every neuron parameter from HBM once
// per timestep (k_ensarray, HBM-bound: (din + dout + 5) words per neuron-step), one workgroup takes one
// ensemble, loads its encoders, biases, decoders and LIF state words into REGISTERS once (10 words per
// neuron at din 3, dout 5 - the 256 CUs' vector register files hold 128 MiB), and runs all B timesteps
// with a single workgroup barrier per step.  HBM traffic drops by the block length (256x); the kernel is
// bound by VALU issue instead.
//
// Per timestep and workgroup:
//   x[d]   = pre-stage row (block buffer, staged in LDS) + alpha[d] * filter_state[xrow[d]]
//   for each of the thread's NPT neurons: J = e.x + bias; LIF step on the packed state word; acc += spike*dec
//   acc[dout] -> sums over the wave -> LDS [parity][dout][wave] -> ONE barrier -> every wave adds the wave sums in the
//   same fixed order (deterministic; all waves hold identical totals)
//   filter_state[r] = a[r]*filter_state[r] + b[r]*total[r]; total[r] is staged for the post stage's row.
// At the end the state words go back to HBM and the decoded values / filter states of the last step go to the
// signal vector (what k_ens_finish does after every step of the per-step plan).
// f32 state words hold -(R - dt) for a refractory neuron (see lif_input_part), f64 ones -R (k_ensarray's fast path).
#pragma once
#include <type_traits>
#include "ssn_launch.hpp"

namespace ssn {

// sum over the 64 lanes of a wave, result valid in lane 63 (fixed order -> deterministic)
__device__ inline float wave_sum_dpp(float v) {
  int x;
#define SSN_DPP_ADD(ctrl, rmask)                                                                             \
  x = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xF, false);                    \
  v += __builtin_bit_cast(float, x);
  SSN_DPP_ADD(0xB1, 0xF)     // quad_perm [1,0,3,2]
  SSN_DPP_ADD(0x4E, 0xF)     // quad_perm [2,3,0,1]
  SSN_DPP_ADD(0x141, 0xF)    // row_half_mirror
  SSN_DPP_ADD(0x140, 0xF)    // row_mirror: every lane of a 16-lane row holds the row sum
  SSN_DPP_ADD(0x142, 0xA)    // row_bcast15 -> rows 1, 3
  SSN_DPP_ADD(0x143, 0xC)    // row_bcast31 -> rows 2, 3: lane 63 = total
#undef SSN_DPP_ADD
  return v;
}
// sum within each 16-lane row, result in every lane of the row
__device__ inline float row_sum_dpp(float v) {
  int x;
#define SSN_DPP_ADD(ctrl)                                                                                    \
  x = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, false);                      \
  v += __builtin_bit_cast(float, x);
  SSN_DPP_ADD(0xB1) SSN_DPP_ADD(0x4E) SSN_DPP_ADD(0x141) SSN_DPP_ADD(0x140)
#undef SSN_DPP_ADD
  return v;
}
// N independent wave sums, stage by stage (result of each in lane 63)
template <int N>
__device__ inline void wave_sum_dpp_n(float* v) {
#define SSN_DPP_STAGE(ctrl, rmask)                                                                            \
  _Pragma("unroll") for (int r = 0; r < N; ++r) {                                                              \
    const int x = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[r]), ctrl, rmask, 0xF, false);      \
    v[r] += __builtin_bit_cast(float, x);                                                                      \
  }
  SSN_DPP_STAGE(0xB1, 0xF) SSN_DPP_STAGE(0x4E, 0xF) SSN_DPP_STAGE(0x141, 0xF) SSN_DPP_STAGE(0x140, 0xF)
  SSN_DPP_STAGE(0x142, 0xA) SSN_DPP_STAGE(0x143, 0xC)
#undef SSN_DPP_STAGE
}
__device__ inline double wave_sum_dpp(double v) {     // parity/test instantiation: plain shuffles, result in every lane
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <int N>
__device__ inline void wave_sum_dpp_n(double* v) {
#pragma unroll
  for (int r = 0; r < N; ++r) v[r] = wave_sum_dpp(v[r]);
}

// ---- packed f32 arithmetic with the VOP3P clamp modifier: result clamped to [0, 1], NaN -> 0 (DX10 clamp mode) ------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ inline f32x2 pk_clamp01(f32x2 x) {
  f32x2 r;
  asm("v_pk_mul_f32 %0, %1, 1.0 op_sel_hi:[1,0] clamp" : "=v"(r) : "v"(x));
  return r;
}
__device__ inline f32x2 pk_mul_clamp01(f32x2 x, f32x2 y) {
  f32x2 r;
  asm("v_pk_mul_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(x), "s"(y));          // (y: a uniform constant pair)
  return r;
}
__device__ inline f32x2 pk_fma_clamp01_vsv(f32x2 x, f32x2 y, f32x2 z) {          // clamp(x * y + z), y a uniform constant pair
  f32x2 r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(x), "s"(y), "v"(z));
  return r;
}
// clamp(x * y + z), z a uniform constant pair, x the RESULT OF A TRANSCENDENTAL (v_log_f32): gfx940-family hardware needs one
// wait state between a transcendental's write and a non-transcendental VALU read of that register, and the compiler's hazard
// recognizer does not look inside inline asm - so the wait state is part of the asm (without it the DOUT = 5 variants, whose
// schedule put the v_log right in front, read the stale register: caught by the sharded-runner f32 test).
__device__ inline f32x2 pk_fma_clamp01_trans_vvs(f32x2 x, f32x2 y, f32x2 z) {
  f32x2 r;
  asm("s_nop 0\n\tv_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(x), "v"(y), "s"(z));
  return r;
}

// Branch-free f32 LIF step, TWO neurons per call in the two halves of 64-bit register pairs, built ONLY from packed
// multiply / add / FMA (v_pk_*_f32: 2 flops per lane per issue slot) plus one v_rcp_f32 per neuron:
// no compare, no select, no integer min / max.  On gfx950 every non-FMA vector instruction (v_cndmask, v_cmp, v_max_i32,
// v_med3 ...) costs a full issue slot of its own per NEURON where a packed one serves two (v_cndmask: five of them - measured,
// tools/valu_issue_rate.hip, profiles/round3_valu_issue_rate.txt), so the selects of nengo's LIF step (SURVEY
// Appendix A.4) are rewritten as exact arithmetic on {0, 1} indicators made with the clamp modifier.
//
// Inside the time loop the state word is w = 1 - V for a neuron that integrates (0 <= w <= 1: the distance to the threshold).
// A refractory neuron holds, instead of a time, what its NEXT integration needs: with rho = R - dt > 0 the refractory time left
// after the coming step, g = exp((rho - dt) / tau_rc) is exp(-delta / tau_rc) of that step (delta = clip(dt - rho, 0, dt)),
// and the word is w = 1 + kappa (g - q), q = exp(-dt / tau_rc), kappa a power of two that maps the range of g - q onto (0, 1].
// nengo's spike time t_spike = dt + tau_rc log1p(-u), u = (V - 1) / (J - 1), then gives g = C1 (1 - u) with
// C1 = exp((tau_ref - dt) / tau_rc): the logarithm at the spike and the exponential at the end of the refractory period cancel,
// g is AFFINE in u, one more step of waiting multiplies it by q, and em = -expm1(-delta / tau_rc) = clip(1 - g, 0, E1),
// E1 = 1 - q, is affine in w.  No polynomial, no logarithm: 11 packed operations per neuron pair (16 with the two interpolants
// this replaces, whose errors - 2.3e-7 and 5e-8 - went with them).  The input current arrives as JE = E1 (J - 1): the bias
// registers hold (bias - 1) E1, the encoder entries are multiplied by E1 as they are loaded (the buffers in HBM are unchanged).
// With h = dt / tau_rc:  a = 1 / (kappa E1), c = a + 1 rounded up, m1 = 1 + kappa E1, A = kappa (C1 - q), B = kappa C1 E1.
//
//   W0 = clamp(w)                 1 - V0  (V0 = 0 while refractory)
//   dl = clamp(c - a w)           em / E1 = clamp((1 - g) / E1): exactly 1 for every integrating neuron (w <= 1; c - a >= 1 in exact
//                                 arithmetic), 0 for one that stays refractory through the step (g >= 1)
//   nmt = clamp(q w - q m1)       kappa (q g - q), > 0 while the neuron stays refractory beyond the next step: its new word is 1 + nmt
//   t  = W0 E1 + JE               E1 (J - V0)
//   U  = t dl - W0                V - 1 = V0 + (J - V0) em - 1
//   spk = clamp(U * 2^100)        1 if V > 1, else 0 (a positive U is at least 2^-53: it is the rounded difference of a
//                                 product >= 2^-6 and a W0 next to it)
//   rc = rcp(JE);  u' = U rc      u / E1.  A neuron that crosses the threshold in this step has 0 <= u <= E1 (the overshoot V - 1 is
//                                 at most (J - 1) em).  A silent neuron feeds rcp whatever its operand is (0, negative: inf, NaN);
//                                 the clamp below turns any of it into a number in [0, 1] (DX10 clamp: NaN -> 0), spk = 0 discards it
//   nu = clamp(A - B u')          kappa (C1 (1 - u) - q) of a spiking neuron: inside [0, A], A <= 1, because tau_ref >= dt
//   Wn = clamp(spk * 2^100 - U)   1 - Vn: voltage of a silent neuron clamped at min_voltage 0, Vn = 0 for a spiking one
//   w' = (Wn + nmt) + spk * nu    (spiking: Wn = 1, nmt = 0; silent: spk = 0 - exact selects, products with 0 / 1)
// Requires dt / tau_rc <= 1/20, tau_ref >= dt and kappa >= 4 (checked by the host planner, lif_affine_kappa: a smaller kappa -
// a refractory period of many steps - leaves g - q too few bits; such models run the per-timestep kernel).
struct LifConstA { float q, nqm1, E1, A, nB, na, c, kq, rkq, tau_rc, rtau_rc; };      // kq = kappa q (prologue), rkq = 1 / (kappa q) (epilogue)
// The same constants as the time loop reads them: every one as a pair of equal halves, the operand form of the packed
// instructions.  (Scalar fields, splat at each use, come out of the optimizer as overlapping two-word loads of neighbouring
// fields, which keep the whole structure in scratch memory once the loop reads it at more places.)
struct LifConstAP { f32x2 q, nqm1, E1, A, nB, na, c; };

// (uniform; evaluated once per launch, in double; kappa: lif_affine_kappa, ssn_launch.hpp - the planner reads it too)
__device__ inline LifConstA lif_const_affine(double dt, double tau_rc, double tau_ref) {
  const double h = dt / tau_rc, q = exp(-h), E1 = -expm1(-h), C1 = exp((tau_ref - dt) / tau_rc);
  const double kappa = lif_affine_kappa(dt, tau_rc, tau_ref);
  LifConstA c;
  const float a = (float)(1.0 / (kappa * E1));
  float ca = a + 1.0f;
  if ((double)ca < (double)a + 1.0) ca = __builtin_bit_cast(float, __builtin_bit_cast(unsigned int, ca) + 1u);      // next float up: c - a >= 1 in exact arithmetic, a full step is 1, never 1 - ulp
  c.na = -a; c.c = ca;
  c.q = (float)q; c.nqm1 = (float)(-q * (1.0 + kappa * E1)); c.E1 = (float)E1;
  c.A = (float)(kappa * (C1 - q)); c.nB = (float)(-kappa * C1 * E1);
  c.kq = (float)(kappa * q); c.rkq = (float)(1.0 / (kappa * q)); c.tau_rc = (float)tau_rc; c.rtau_rc = (float)(1.0 / tau_rc);
  return c;
}

// The step in two halves: lif_state_part needs only the state word, lif_input_part is what needs J.  The time loop runs the
// state half of some groups one timestep ahead, INSIDE the waits of the cross-wave sum (SSN_BLOCK_HOIST_*).
// (Measured and dropped in round 3: the state half of ALL of a thread's neurons as one lump in the tail of the previous timestep,
// behind the wait for the wave sums - where it overlaps nothing - or, the older wave of each SIMD, in front of the barrier, 40 more
// registers: 2.90 - 2.92 ms per 1000 steps either way against 2.91 - 2.92 with the halves back to back, same box; alternating
// s_setprio between the two waves of a SIMD: 3.21 ms.)
// (its instructions one by one, for the time loop's tail, which places them between the steps of the cross-wave sum)
__device__ inline f32x2 lif_state_dl(f32x2 w, f32x2 na, f32x2 ca) {
  return pk_fma_clamp01_vsv(w, (f32x2)(na), (f32x2)(ca));                   // clamp(c - a w)
}
__device__ inline f32x2 lif_state_nmt(f32x2 w, f32x2 q, f32x2 nqm1) {
  return pk_fma_clamp01_vsv(w, (f32x2)(q), (f32x2)(nqm1));                  // clamp(q w - q m1)
}
__device__ inline void lif_state_part(f32x2 w, const LifConstAP& c, f32x2& W0, f32x2& dl) {
  W0 = pk_clamp01(w);
  dl = lif_state_dl(w, c.na, c.c);
}
// The input half in three pieces, so that a wave whose neurons are all silent in a timestep can leave out the spike-time
// arithmetic (round 4): lif_spike_test produces U = V - 1 and the spike indicators; lif_finish_spiking
// is the rest of lif_input_part; lif_finish_silent is what that rest computes when every indicator is 0 - bit for bit:
// Wn = clamp(0 * 2^100 - U) = clamp(-U), w' = fma(0, nu, Wn + nmt) = Wn + nmt (nu is a number in [0, 1] after its clamp, so
// 0 * nu = +0, and Wn + nmt >= 0).
__device__ inline f32x2 lif_spike_test(f32x2 JE, f32x2 W0, f32x2 dl, const LifConstAP& c, f32x2 big, f32x2& U) {
  const f32x2 t = __builtin_elementwise_fma(W0, c.E1, JE);
  U = __builtin_elementwise_fma(t, dl, -W0);
  return pk_mul_clamp01(U, big);
}
__device__ inline void lif_finish_spiking(f32x2 JE, f32x2& w, f32x2 U, f32x2 nmt, f32x2 spk, const LifConstAP& c, f32x2 big) {
  f32x2 rc;
  rc.x = __builtin_amdgcn_rcpf(JE.x);
  rc.y = __builtin_amdgcn_rcpf(JE.y);
  f32x2 Wn, u, nu;
  asm("v_pk_fma_f32 %0, %2, %3, %4 neg_lo:[0,0,1] neg_hi:[0,0,1] clamp\n\t"
      "v_pk_mul_f32 %1, %4, %5"
      : "=&v"(Wn), "=v"(u)
      : "v"(spk), "s"(big), "v"(U), "v"(rc));
  asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(nu) : "v"(u), "s"((f32x2)(c.nB)), "v"((f32x2)(c.A)));
  w = __builtin_elementwise_fma(spk, nu, Wn + nmt);
}
__device__ inline void lif_finish_silent(f32x2& w, f32x2 U, f32x2 nmt) {
  f32x2 Wn;
  asm("v_pk_mul_f32 %0, %1, -1.0 op_sel_hi:[1,0] clamp" : "=v"(Wn) : "v"(U));          // clamp(-U)
  w = Wn + nmt;
}
// (nmt: lif_state_nmt of the word, here or - hoisted groups of the pipelined tail - one timestep ahead)
__device__ inline f32x2 lif_input_part(f32x2 JE, f32x2& w, f32x2 W0, f32x2 dl, f32x2 nmt, const LifConstAP& c, f32x2 big) {
  f32x2 U;
  const f32x2 spk = lif_spike_test(JE, W0, dl, c, big, U);
  // Wn = clamp(spk * 2^100 - U) sits between the reciprocals and their first reader: the wait state a non-transcendental reader
  // of a transcendental's result needs is filled by an instruction that has to be issued anyway (the compiler's hazard recognizer
  // does not look inside inline asm, so the order is fixed by ONE asm statement: Wn, then u' = U * rc)
  lif_finish_spiking(JE, w, U, nmt, spk, c, big);
  return spk;
}
// HBM state word (s >= 0: voltage; s < 0: -(R - dt)) <-> loop word, in the forms that keep relative accuracy as R - dt -> 0:
// kappa (g - q) = kappa q expm1(rho / tau_rc), rho = tau_rc log1p((w - 1) / (kappa q)) - never exp / log of a number next to 1
__device__ inline float lif_word_in(float s, float kq, float rtau_rc) {
  return s < 0.0f ? __builtin_fmaf(kq, expm1f(-s * rtau_rc), 1.0f) : 1.0f - s;
}
__device__ inline float lif_word_out(float w, float rkq, float tau_rc) {
  return w > 1.0f ? -(tau_rc * log1pf((w - 1.0f) * rkq)) : 1.0f - w;
}

__device__ inline float bits_f(unsigned int x) { return __builtin_bit_cast(float, x); }
__device__ inline unsigned int f_bits(float x) { return __builtin_bit_cast(unsigned int, x); }

#ifdef SSN_BLOCK_STAMPS
// diagnostic build only (make F32_EXTRA=-DSSN_BLOCK_STAMPS, tools/block_stamps.py): shader-clock stamps (s_memtime) between the
// sections of a timestep of the f32 time loop, summed per wave and added up over all waves at the end of the launch:
//   [0] input assembly (LDS row read, v_readlane of the filter states)   [1] neuron groups (encode, LIF step, decode)
//   [2] wave reduction + publication of the wave sums in LDS              [3] wait at the workgroup barrier
//   [4] totals over the waves, filter update, hand-off to the post stage  [5] wave-timesteps counted
//   [6] / [7] s_memtime / s_memrealtime ticks of workgroup 0's time loop (shader clock = 100 MHz * [6] / [7])
//   [8] the part of [4] from the barrier to the totals over the waves (LDS read of the wave sums + row sum); the rest of [4]
//       is the filter update, the next timestep's input (pipelined loop: there [0] is empty) and the hand-off
// (callers pass room for 9 words)
__device__ unsigned long long g_block_stamps[9];
inline hipError_t read_block_stamps(unsigned long long* out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_block_stamps), sizeof(unsigned long long) * 9);
  if (e == hipSuccess && reset) {
    const unsigned long long z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_block_stamps), z, sizeof z);
  }
  return e;
}
#define SSN_BSTAMP(var)                                                                          \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var) :: "memory");                \
    __builtin_amdgcn_sched_barrier(0);                                                           \
  } while (0)
#define SSN_BSTAMP_ADD(i, a, b) bst[i] += (b) - (a)
#else
#define SSN_BSTAMP(var) do {} while (0)
#define SSN_BSTAMP_ADD(i, a, b) do {} while (0)
#endif

#ifndef SSN_BLOCK_SKIP
#define SSN_BLOCK_SKIP 0      // silent-slot modes of the f32 neuron rounds (compile-time, default off: see the time loop)
#endif
// The f32 time loop's tail, pipelined (variants with five or more neuron groups; 0 restores the plain loop):
//   SSN_BLOCK_PIPE     the next timestep's input row is read from LDS in front of the wave reduction and x of timestep jj + 1 is
//                      assembled at the end of timestep jj, so that no LDS round trip sits between the totals and the first encode FMA
//   SSN_BLOCK_HOIST_A  neuron groups whose state half of timestep jj + 1 runs between the publication of the wave sums and the barrier
//   SSN_BLOCK_HOIST_B  ... between the LDS read of the wave sums and the wait for it
//   SSN_BLOCK_HOIST_D  ... between the filter update and the v_readlane that reads it
//   SSN_BLOCK_HOIST_NMT  1: the state half is W0, dl and the stay-refractory term nmt (three packed operations, six registers from
//                      the tail to the group's round of the next timestep); 0: W0 and dl only (two operations, four registers)
// block_hoist() cuts the counts to what the variant's register budget (512 / waves per SIMD) leaves.  Outputs are bit for bit
// those of the plain loop for every setting.  Measured at (512, 20, LDS), ms per bench step (profiles/lif_affine_placements.txt):
// nothing hoisted 2.57 - 2.58; D 1, A 2, B 4 2.52 - 2.53, with nmt 2.51; D 0 2.56 - 2.58, D 2 2.60 - 2.62; B 2 or 6 2.54 - 2.55.
// (The five-operation state half of the polynomial step also ran two groups instruction by instruction between the four DPP steps
// of the row sum - profiles/block_tail_placements.txt; rewritten for W0 / dl of four groups it measured 2.53 - 2.55 against
// 2.52 - 2.53 without: removed.)
#ifndef SSN_BLOCK_PIPE
#define SSN_BLOCK_PIPE 1
#endif
#ifndef SSN_BLOCK_HOIST_A
#define SSN_BLOCK_HOIST_A 2
#endif
#ifndef SSN_BLOCK_HOIST_B
#define SSN_BLOCK_HOIST_B 4
#endif
#ifndef SSN_BLOCK_HOIST_D
#define SSN_BLOCK_HOIST_D 1
#endif
#ifndef SSN_BLOCK_HOIST_NMT
#define SSN_BLOCK_HOIST_NMT 1
#endif
struct BlockHoist { int a, b, d; };
constexpr BlockHoist block_hoist(bool pipe, int tpb, int ng) {
  if (!pipe || SSN_BLOCK_SKIP != 0) return {0, 0, 0};
  const int room = tpb <= 512 && ng >= 10 ? ng : 0;         // only two waves per SIMD at ten groups have registers to spare: 768 threads
                                                            // spill, (512, 10) would drop from three waves per SIMD to two
  const int d = SSN_BLOCK_HOIST_D < room ? SSN_BLOCK_HOIST_D : room;
  const int b = SSN_BLOCK_HOIST_B < room - d ? SSN_BLOCK_HOIST_B : room - d;
  const int a_ = SSN_BLOCK_HOIST_A < room - d - b ? SSN_BLOCK_HOIST_A : room - d - b;
  return {a_, b, d};
}

// Neurons are dealt to threads in groups of PK adjacent neurons (PK = 2 for f32: one 64-bit register pair,
// 1 for f64): neuron index of (group g, thread tid, component c) = (g * nthr + tid) * PK + c - coalesced.
//
// Cross-lane sums (f32).  Per timestep a wave owes DOUT sums over its 64 lanes, and every wave then needs the DOUT
// totals over all waves for the filter update and the next input.  Both steps are kept off the scalar unit and off
// per-row instruction sequences:
//   * in the wave: four values at once - two v_permlane32_swap + add fold lanes 32..63 onto 0..31 for two value pairs,
//     one v_permlane16_swap + add leaves the four values in the four 16-lane rows, four DPP steps finish all four rows
//     together (gfx950's swap instructions; a fifth value takes the plain six-step DPP sum): 17 instead of 30 steps;
//   * across waves: wave w leaves value r in LDS slot r * 16 + w; after the one barrier of the timestep lane l of every
//     wave reads slot l, so a four-step DPP row sum gives row r of EVERY wave the total of value r in fixed order
//     (identical in all waves: deterministic).  The totals stay "lane-distributed" (row r of a register = decoded row
//     r): the Lowpass update of the recurrent filter states is ONE v_fma on that register with per-lane constants, and
//     only the (at most DIN) states the next input needs are broadcast with v_readlane.
// TAP: the tapped twin (neuron probes on members of the array, BlockArgs::tap_slot): the workgroup of a tapped ensemble also
// stores amp * spike of the tapped neurons into the timestep's row of the block buffer - global stores inside the time loop
// of those workgroups only (a wave-uniform test; every other workgroup of the launch runs the plain loop's instructions).
// Its own instantiation, as SPLIT: an array without taps launches the kernel it always launched.
template <typename T, int DIN, int DOUT, int NPT, int TPB, int LDSW, int SPLIT = 0, int TAP = 0>      // LDSW: 0 all parameters in registers | DIN: the encoder rows in LDS
__global__ __launch_bounds__(TPB) void k_ens_block(BlockArgs<T> a) {   // SPLIT: an ensemble over a.P member workgroups (own instantiation: the plain kernel's loop stays as it is)
  static_assert(!(SPLIT && TAP), "the split kernel has no tapped form");
  constexpr bool ENC_LDS = LDSW == DIN;
  // (Encoders AND bias in LDS - rows as long as the padded neuron count, 160 000 of the CU's 163 840 bytes at n = 10 000 -
  //  were built and measured in round 2: (768, 14) 3.68 ms and (1024, 10) 3.64 ms per 1000 timesteps of config 2 against
  //  3.49 for (512, 20) with the bias in registers: removed.)
  static_assert(LDSW == 0 || LDSW == DIN, "LDSW");
  extern __shared__ __align__(16) unsigned char ssn_block_dyn[];
  T* const e_lds = reinterpret_cast<T*>(ssn_block_dyn);       // ENC_LDS: encoder rows [DIN][cap]
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int PK = F32 ? 2 : 1;
  constexpr int NG = NPT / PK;
  static_assert(NPT % PK == 0, "f32 variants handle neuron pairs");
  constexpr bool PIPE = F32 && NG >= 5 && SSN_BLOCK_PIPE != 0;     // (variants with one to three groups keep the plain loop: their
                                                                   //  1024-thread workgroups have no register to spare for the row)
  constexpr BlockHoist HO = block_hoist(PIPE, TPB, NG);
  constexpr int HD = HO.d, HA = HO.a, HB = HO.b, HT = HD + HA + HB;      // hoisted groups: [0, HD) | [HD, HD + HA) | [HD + HA, HT)
  constexpr bool HNMT = SSN_BLOCK_HOIST_NMT != 0;                        // the hoisted groups carry their nmt along
  using G = typename std::conditional<F32, f32x2, T>::type;   // one group of neurons
  constexpr int DP = DOUT <= 4 ? 4 : 8;
  // split ensembles: P consecutive workgroups are the members of ensemble k (f32, DOUT <= 4 only - the planner sees to it)
  static_assert(!SPLIT || (sizeof(T) == 4 && DOUT <= 4), "split ensembles: f32, at most four decoded rows");
  const int P = SPLIT ? a.P : 1;
  const int k = P > 1 ? (int)blockIdx.x / P : (int)blockIdx.x;
  const int member = P > 1 ? (int)blockIdx.x - k * P : 0;
  const int noff = member * a.n_member;                        // first neuron of this member's slice
  const int n_loc = P > 1 ? max(0, min(a.n_member, a.n_pad - noff)) : a.n_pad;
  const int tid = threadIdx.x;
  const int nthr = NG == 1 ? (int)blockDim.x : TPB;       // variants with more than one group always run full workgroups
  const int lane = tid & 63, wave = tid >> 6;
  const size_t row = (size_t)a.n_pad;
  const T* __restrict__ enc = a.enc + (size_t)k * DIN * row + noff;
  const T* __restrict__ bias = a.bias + (size_t)k * row + noff;
  T* __restrict__ Sp = a.S + (size_t)k * row + noff;
  const NeuronParams<T> np = a.np;
  const LifMath<T> lm(np);
  // tapped twin: this ensemble's row of destination signals per device column (workgroup-uniform; nullptr: no tap here)
  const int* tcol = nullptr;
  if constexpr (TAP != 0) {
    const int tslot = a.tap_slot[k];
    if (tslot >= 0) tcol = a.tap_col + (size_t)tslot * row;
  }
  // (uniform values: readfirstlane moves them to scalar registers, where the packed instructions of the time loop can take
  //  them as their one constant-bus operand)
  auto uni = [](float v) { return bits_f(__builtin_amdgcn_readfirstlane(f_bits(v))); };
  const LifConstA lc0 = lif_const_affine((double)np.dt, (double)np.tau_rc, (double)np.tau_ref);
  auto uni2 = [&](float v) { const float u = uni(v); return (f32x2){u, u}; };
  const LifConstAP lc = {uni2(lc0.q), uni2(lc0.nqm1), uni2(lc0.E1), uni2(lc0.A), uni2(lc0.nB), uni2(lc0.na), uni2(lc0.c)};
  const float lcE1 = uni(lc0.E1), lcKq = uni(lc0.kq), lcRkq = uni(lc0.rkq), lcTau = uni(lc0.tau_rc), lcRtau = uni(lc0.rtau_rc);
  const f32x2 big = {0x1p100f, 0x1p100f};

  // ---- parameters and state of this thread's neurons -> registers ---------------------------------------------
  G e[ENC_LDS ? 1 : NG][DIN], b[NG], s[NG], dc[NG][DOUT];
  // LDS rows: as long as the variant's capacity (compile-time strides).
  constexpr int cap = (NG == 1 ? 1024 : TPB) * NPT;
  // one LDS base address per parameter row; a group's entry is a compile-time offset from it (the opaque asm keeps the
  // compiler from hoisting one address register per (group, row) out of the time loop: 28 registers at 7 groups)
  int lrow[LDSW > 0 ? LDSW : 1];           // (element offsets, not pointers: a pointer that went through the asm would be
#pragma unroll                             //  dereferenced with flat loads - 64-bit addresses, and the LDS aperture check)
  for (int d = 0; d < (LDSW > 0 ? LDSW : 1); ++d) {
    lrow[d] = d * cap + tid * PK;
    asm volatile("" : "+v"(lrow[d]));
  }
  auto lds_group = [&](int d, int g) -> const G* {
    return reinterpret_cast<const G*>(e_lds + lrow[d] + g * nthr * PK);
  };
  // Straight-line loads, no per-neuron branches (which cost the register allocator its view of the long live ranges):
  // rows are zero-padded to n_pad (a multiple of 4 elements) on upload, so a whole group is read whenever it starts
  // inside the padded row; groups past it read group 0 and are multiplied by 0.
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int i0 = (g * nthr + tid) * PK;
    const bool in = i0 < n_loc;
    const int ii = in ? i0 : 0;
    const T msk = in ? T(1) : T(0);
    auto ld = [&](const T* p) -> G { if constexpr (F32) return *reinterpret_cast<const f32x2*>(p) * msk; else return *p * msk; };
#pragma unroll
    for (int d = 0; d < DIN; ++d) {
      G ev = ld(enc + d * row + ii);
      if constexpr (F32) ev = ev * lcE1;                   // the encode FMAs produce JE = E1 (J - 1)
      if constexpr (ENC_LDS) *reinterpret_cast<G*>(e_lds + d * cap + i0) = ev; else e[g][d] = ev;
    }
    b[g] = ld(bias + ii);
    s[g] = ld(Sp + ii);
    if constexpr (F32) {                                   // the time loop's forms: E1 (J - 1), distance to the threshold (lif_state_part / lif_input_part)
      b[g] = (b[g] - 1.0f) * lcE1;
      s[g] = (f32x2){lif_word_in(s[g].x, lcKq, lcRtau), lif_word_in(s[g].y, lcKq, lcRtau)};
    }
    if (a.dec_neuron_major) {
      const T* dp = a.dec + ((size_t)k * row + noff + ii) * DP;
#pragma unroll
      for (int r = 0; r < DOUT; ++r) {
        if constexpr (F32) dc[g][r] = (f32x2){dp[r], dp[DP + r]} * msk; else dc[g][r] = dp[r] * msk;
      }
    } else {
      const T* dp = a.dec + (size_t)k * DOUT * row + noff + ii;
#pragma unroll
      for (int r = 0; r < DOUT; ++r) dc[g][r] = ld(dp + r * row);
    }
  }

  // ---- LDS: wave sums (two parities), and the block-buffer traffic of CH timesteps at a time so that no global
  //      memory operation sits inside the time loop (a workgroup barrier waits for every outstanding one) ----
  constexpr int CH = 32;                     // timesteps per input/output chunk (static LDS stays under 2 KB)
  constexpr int XP = 4;                      // words per timestep of inputs (DIN <= 4): one 16-byte LDS read
  constexpr int RW = DOUT <= 4 ? 64 : 128;   // wave-sum slots per parity: [r][16 waves]
  __shared__ __align__(16) T red[2][RW];
  __shared__ __align__(16) T xs[CH][XP];
  __shared__ T os[CH][DOUT];
  __shared__ int s_dst[DOUT];
  __shared__ int s_out[DOUT];
  for (int i = tid; i < 2 * RW; i += nthr) (&red[0][0])[i] = T(0);     // waves that do not exist add 0
  if (tid < DOUT) { s_dst[tid] = a.didx[(long long)k * DOUT + tid]; s_out[tid] = a.rowout[(long long)k * DOUT + tid] ? 1 : 0; }
  const T* __restrict__ xbase = a.xrows + (size_t)a.row0 * a.n_sig + a.x_off + (long long)k * DIN;

  // ---- per-row constants.  f32: lane-distributed - register 0 holds decoded row (lane >> 4), register 1 row 4 -----
  //      f64 (parity / small ensembles): uniform arrays, as the per-timestep kernel computes them
  T fs[F32 ? 1 : DOUT], la[F32 ? 1 : DOUT], lb[F32 ? 1 : DOUT], tot[F32 ? 1 : DOUT];
  float F0 = 0.0f, F1 = 0.0f, la0 = 0.0f, lb0 = 0.0f, la1 = 0.0f, lb1 = 0.0f, v0 = 0.0f, v1 = 0.0f;
  T xa[DIN];
  int xr[DIN];
#pragma unroll
  for (int d = 0; d < DIN; ++d) {
    xr[d] = a.xrow[(long long)k * DIN + d];
    xa[d] = xr[d] >= 0 ? a.xalpha[(long long)k * DIN + d] : T(0);
  }
  if constexpr (F32) {
    const int r0 = lane >> 4;
    if (r0 < DOUT) {
      const long long i = (long long)k * DOUT + r0;
      const int st = a.lp_state[i];
      if (st >= 0) { F0 = a.sig[st]; la0 = a.lp_a[i]; lb0 = a.lp_b[i]; }
    }
    if (DOUT > 4) {
      const long long i = (long long)k * DOUT + 4;
      const int st = a.lp_state[i];
      if (st >= 0) { F1 = a.sig[st]; la1 = a.lp_a[i]; lb1 = a.lp_b[i]; }
    }
  } else {
#pragma unroll
    for (int r = 0; r < DOUT; ++r) {
      const long long i = (long long)k * DOUT + r;
      const int st = a.lp_state[i];
      fs[r] = st >= 0 ? a.sig[st] : T(0);
      la[r] = st >= 0 ? a.lp_a[i] : T(0);
      lb[r] = st >= 0 ? a.lp_b[i] : T(0);
      tot[r] = T(0);
    }
  }
  // f32: where this lane's wave sums go (slot r * 16 + wave) and which filter states feed the inputs
  int wslot = -1;
  if constexpr (F32) {
    if constexpr (DOUT >= 4) {
      // after the swap reduction the rows of the 4-value register hold values 0, 2, 1, 3; value 4 sits in lane 63
      const int rv = (lane >> 4) == 1 ? 2 : ((lane >> 4) == 2 ? 1 : (lane >> 4));
      if ((lane & 15) == 0) wslot = rv * 16 + wave;
      if (DOUT == 5 && lane == 63) wslot = 64 + wave;
    }
  }

  constexpr int ILE = F32 ? (SSN_BLOCK_IL < NG ? SSN_BLOCK_IL : NG) : 1;      // groups stepped side by side (see the time loop)
  G en[ILE][LDSW > 0 ? LDSW : 1];            // ENC_LDS: encoders (and bias) of the groups about to be processed
  if constexpr (ENC_LDS) {
#pragma unroll
    for (int u = 0; u < ILE; ++u)
#pragma unroll
      for (int d = 0; d < LDSW; ++d) en[u][d] = *lds_group(d, u);
  }
#ifdef SSN_BLOCK_STAMPS
  unsigned long long bst[6] = {0, 0, 0, 0, 0, 0}, bt0 = 0, bt1 = 0, bt2 = 0, bt3 = 0, bt4 = 0, bt5 = 0, bt6 = 0, bm0 = 0, br0 = 0;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(bm0), "=s"(br0) :: "memory");
#endif
  unsigned int n_slots = 0, n_silent = 0;      // (wave-uniform: scalar registers)
  T x[DIN];
  int xl[DIN];                                 // lane of F0 that holds the state input d reads (uniform: a scalar register, read once)
#pragma unroll
  for (int d = 0; d < DIN; ++d) xl[d] = __builtin_amdgcn_readfirstlane((xr[d] & 3) << 4);
  // f32 input: pre-stage row + alpha * the filter state it reads - row xr[d] of the lane-distributed registers (uniform lane index)
  auto assemble_x = [&](const float4 xv) {
    const float xin[4] = {xv.x, xv.y, xv.z, xv.w};
    float f1 = 0.0f;
    if constexpr (DOUT > 4) f1 = bits_f(__builtin_amdgcn_readlane(f_bits(F1), 0));
#pragma unroll
    for (int d = 0; d < DIN; ++d) {
      const float f0 = bits_f(__builtin_amdgcn_readlane(f_bits(F0), xl[d]));
      float st = f0;                                            // (a v_cndmask costs five issue slots: only where a fifth row exists)
      if constexpr (DOUT > 4) st = xr[d] >= 4 ? f1 : f0;
      x[d] = __builtin_fmaf(xa[d], st, xin[d]);                 // (xa = 0 where no state feeds the input)
    }
  };
  // pipelined tail: the state half (W0, dl) of the hoisted groups' NEXT step, computed in the waits of the cross-wave sum
  // (the state word is final when a group's round ends; after the last timestep of the launch the values are dropped)
  f32x2 W0h[HT > 0 ? HT : 1], dlh[HT > 0 ? HT : 1], nmth[HT > 0 ? HT : 1];
  auto hoist_state = [&](int g) {
    lif_state_part(s[g], lc, W0h[g], dlh[g]);
    if constexpr (HNMT) nmth[g] = lif_state_nmt(s[g], lc.q, lc.nqm1);
  };
  if constexpr (HT > 0) {
#pragma unroll
    for (int g = 0; g < HT; ++g) hoist_state(g);
  }
  for (int j0 = 0; j0 < a.B; j0 += CH) {
    const int cn = min(CH, a.B - j0);
    __syncthreads();                         // previous chunk: every wave is past its last xs read / os write
    if (j0 > 0 && member == 0) {             // hand the previous chunk's decoded rows to the post stage
      for (int i = tid; i < CH * DOUT; i += nthr) {
        const int jj = i / DOUT, r = i - jj * DOUT;
        if (s_out[r]) a.bsig[(size_t)(a.row0 + j0 - CH + jj) * a.n_sig + s_dst[r]] = os[jj][r];
      }
    }
    for (int i = tid; i < cn * DIN; i += nthr) {
      const int jj = i / DIN, d = i - jj * DIN;
      xs[jj][d] = xbase[(size_t)(j0 + jj) * a.n_sig + d];
    }
    __syncthreads();
    if constexpr (PIPE) {                    // the chunk's first input (every later one is assembled in the tail of the timestep before it)
      assemble_x(*(const float4*)xs[0]);
    }

    for (int jj = 0; jj < cn; ++jj) {
      SSN_BSTAMP(bt0);
      if constexpr (SPLIT != 0) {
        if (P > 1 && wave == 0 && (lane & 15) == 0) {        // split ensemble: own words of the NEXT exchange buffer back to the sentinel
          unsigned int* const rst = a.xslots + (size_t)k * 64 + (size_t)((j0 + jj + 1) % 3) * ((size_t)a.K * 64) + member * 4 + (lane >> 4);
          const unsigned int sent = BLOCK_XCHG_SENTINEL;
          asm volatile("global_store_dword %0, %1, off sc0 sc1" :: "v"(rst), "v"(sent) : "memory");
        }
      }
      if constexpr (PIPE) {
        // (x was assembled in the tail of the timestep before)
      } else if constexpr (F32) {
        assemble_x(*(const float4*)xs[jj]);
      } else {
        T xin[XP];
        *(double2*)xin = *(const double2*)xs[jj]; *(double2*)(xin + 2) = *(const double2*)(xs[jj] + 2);
#pragma unroll
        for (int d = 0; d < DIN; ++d) {
          T st = T(0);
#pragma unroll
          for (int r = 0; r < DOUT; ++r) st = xr[d] == r ? fs[r] : st;
          x[d] = xr[d] >= 0 ? xin[d] + xa[d] * st : xin[d];
        }
      }
      SSN_BSTAMP(bt1);
      G accg[DOUT];
#pragma unroll
      for (int r = 0; r < DOUT; ++r) accg[r] = G(0);
      // ENC_LDS: a thread reads back only the entries it wrote itself (no barrier needed); the next group's
      // encoders are requested one group ahead so the LDS latency hides under this group's arithmetic
      // Groups are stepped IL at a time: each group's LIF step is one long dependent chain (~30 packed operations, a
      // reciprocal and a logarithm), and with two or three waves per SIMD the hardware alone does not cover its latency -
      // measured 6.8 cycles per vector instruction with one chain per wave against 4.4 issue-bound.  Beyond IL the chains
      // are kept apart (scheduling barrier): more interleaving only costs registers.
      constexpr int IL = ILE;
#pragma unroll
      for (int g0 = 0; g0 < NG; g0 += IL) {
        G J[IL], spk[IL];
#pragma unroll
        for (int u = 0; u < IL; ++u) {
          const int g = g0 + u < NG ? g0 + u : NG - 1;       // (a last, partial round: the surplus slots repeat its last group and are discarded)
          J[u] = b[g];
#pragma unroll
          for (int d = 0; d < DIN; ++d) {
            if constexpr (ENC_LDS) J[u] += en[u][d] * x[d];
            else J[u] += e[g][d] * x[d];
          }
        }
        if constexpr (ENC_LDS) {
          // the groups' LDS operands are consumed: request the next groups' into the same registers now - they arrive
          // under this round's neuron arithmetic (the last round requests round 0: the next timestep's first operands)
#pragma unroll
          for (int u = 0; u < IL; ++u) {
            if (g0 + u >= NG) continue;
            asm volatile("" : "+v"(J[u]));
            const int gn = g0 + IL + u < NG ? g0 + IL + u : (g0 + IL + u) % IL;
#pragma unroll
            for (int d = 0; d < LDSW; ++d) en[u][d] = *lds_group(d, gn);
          }
        }
        // (SSN_BLOCK_SKIP 1 and 2 were measured slower than the plain loop in round 4: see the comments below and DESIGN.md section 3.1)
        // f32: a wave's neurons of this round are often ALL silent - the host deals neurons to (wave, round) slots by the part
        // of the oscillator's cycle in which they can fire (Sim::reorder_block_neurons), so that whole slots fall silent together -
        // and a silent slot needs neither the spike time (two v_rcp, two v_log and two packed operations per neuron pair) nor
        // the decode: 6 of a pair's 22 packed and all 4 of its transcendental instructions.  The branch is wave-uniform.
        // SSN_BLOCK_SKIP == 2: slots AT REST are left out altogether.  A neuron whose input current is <= 0 and whose state word is
        // exactly 1 (V = 0, not refractory) leaves the step as it entered it, bit for bit: W0 = 1, the integration time is a full
        // step, U = J * em - 1 < 0, no spike, Wn = clamp(1 - J * em) = 1, nmt = 0, w' = 1 - and adds +0 to every decoded sum.  The
        // test costs 8 packed / plain instructions per round: r = clamp(J) + (w - 1)^2 over the slot's neurons is 0 only then.
        bool at_rest = false;
        if constexpr (F32 && SSN_BLOCK_SKIP == 2) {
          ++n_slots;
          f32x2 r2 = {0.0f, 0.0f};
#pragma unroll
          for (int u = 0; u < IL; ++u) {
            if (g0 + u >= NG) continue;
            f32x2 pj;
            asm("v_pk_add_f32 %0, %1, %2 clamp" : "=v"(pj) : "v"(J[u]), "s"(lc.E1));      // clamp(E1 J): J[] holds E1 (J - 1)
            const f32x2 q = s[g0 + u] - 1.0f;
            r2 += __builtin_elementwise_fma(q, q, pj);
          }
          at_rest = __builtin_amdgcn_ballot_w64(__builtin_bit_cast(unsigned long long, r2) != 0ull) == 0ull;
          if (at_rest) ++n_silent;
        }
        if constexpr (F32 && SSN_BLOCK_SKIP == 1) {
          ++n_slots;
          f32x2 Uu[IL], nm[IL];
          f32x2 any2 = {0.0f, 0.0f};
#pragma unroll
          for (int u = 0; u < IL; ++u) {
            const int g = g0 + u < NG ? g0 + u : NG - 1;
            f32x2 W0, dl;
            lif_state_part(s[g], lc, W0, dl);
            nm[u] = lif_state_nmt(s[g], lc.q, lc.nqm1);
            spk[u] = lif_spike_test(J[u], W0, dl, lc, big, Uu[u]);
            if (g0 + u < NG) any2 += spk[u];
          }
          if (__builtin_amdgcn_ballot_w64(any2.x + any2.y != 0.0f) != 0ull) {
#pragma unroll
            for (int u = 0; u < IL; ++u)
              if (g0 + u < NG) lif_finish_spiking(J[u], s[g0 + u], Uu[u], nm[u], spk[u], lc, big);
            // the decode belongs to this branch (spk is 0 or 1: exact adds) - the scheduler interleaves its independent FMAs
            // with the rcp -> log chains above; behind the branch the compiler turned a skipped decode into 80 v_cndmask
#pragma unroll
            for (int u = 0; u < IL; ++u) {
              if (g0 + u >= NG) continue;
#pragma unroll
              for (int r = 0; r < DOUT; ++r) accg[r] = __builtin_elementwise_fma(spk[u], dc[g0 + u][r], accg[r]);
            }
          } else {
#pragma unroll
            for (int u = 0; u < IL; ++u)
              if (g0 + u < NG) lif_finish_silent(s[g0 + u], Uu[u], nm[u]);
            ++n_silent;
          }
        }
        if (!at_rest) {
#pragma unroll
        for (int u = 0; u < IL; ++u) {
          const int g = g0 + u;
          if (g >= NG) continue;
          if constexpr (F32 && SSN_BLOCK_SKIP == 1) {
            // (stepped above)
          } else if constexpr (F32) {
            f32x2 W0, dl, nmt;
            if (g < HT) { W0 = W0h[g < HT ? g : 0]; dl = dlh[g < HT ? g : 0]; }      // (computed in the tail of the timestep before)
            else lif_state_part(s[g], lc, W0, dl);
            if (HNMT && g < HT) nmt = nmth[g < HT ? g : 0];
            else nmt = lif_state_nmt(s[g], lc.q, lc.nqm1);
            spk[u] = lif_input_part(J[u], s[g], W0, dl, nmt, lc, big);
          } else {
            // packed state word -> nengo's LIF step, operation for operation k_ensarray's fast path
            const T sw = s[g];
            T V = sw < T(0) ? T(0) : sw;
            T R = (sw < T(0) ? -sw : T(0)) - np.dt;
            T delta = np.dt - R;
            delta = delta < T(0) ? T(0) : (delta > np.dt ? np.dt : delta);
            V = V - (J[u] - V) * lm.decay(delta);
            spk[u] = T(0);
            if (V > T(1)) {
              const T t_spike = np.dt + np.tau_rc * lm.spike_time_term(V, J[u]);
              R = np.tau_ref + t_spike;
              V = T(0);
              spk[u] = T(1);
            } else if (V < T(0)) {
              V = T(0);
            }
            s[g] = R > np.dt ? -R : V;
          }
        }
#pragma unroll
        for (int u = 0; u < IL; ++u) {
          const int g = g0 + u;
          if (g >= NG) continue;
          // the state word is final HERE: without this the compiler sinks the rcp / log half of every group's step to the
          // end of the timestep and keeps its operands live until then
          if constexpr (F32) asm volatile("" : "+v"(s[g]));
          if constexpr (TAP != 0) {
            // spk is 0 or 1: amp * spk is exact.  The row of the block buffer, addressed as the hand-off of the decoded rows
            // addresses it; the destinations are looked up here, not kept in registers across the time loop
            if (tcol) {
              const int i0 = (g * nthr + tid) * PK;
              T* const trow = a.bsig + (size_t)(a.row0 + j0 + jj) * a.n_sig;
              if (i0 < n_loc) {
                if constexpr (F32) {
                  const int2 d = *reinterpret_cast<const int2*>(tcol + i0);
                  const f32x2 val = spk[u] * a.tap_amp;
                  if (d.x >= 0) trow[d.x] = val.x;
                  if (d.y >= 0) trow[d.y] = val.y;
                } else {
                  const int d = tcol[i0];
                  if (d >= 0) trow[d] = spk[u] * a.tap_amp;
                }
              }
            }
          }
          if constexpr (F32 && SSN_BLOCK_SKIP == 1) continue;      // (decoded inside the spiking branch above)
#pragma unroll
          for (int r = 0; r < DOUT; ++r) {           // spk is 0 or 1: exact add
            if constexpr (F32) accg[r] = __builtin_elementwise_fma(spk[u], dc[g][r], accg[r]);
            else accg[r] = fma(spk[u], dc[g][r], accg[r]);
          }
        }
        }
#ifndef SSN_BLOCK_NO_SCHED_BARRIER
        if constexpr (F32) __builtin_amdgcn_sched_barrier(0);
#endif
      }
      const int par = jj & 1;
      SSN_BSTAMP(bt2);
      if constexpr (F32) {
        // pipelined: the next timestep's input row, requested HERE - in front of the wave reduction and the barrier, where its
        // latency lies under the reduction (xs is written once per chunk and fenced by the chunk's own barriers; the compiler
        // may not move an LDS read across s_barrier itself).  The chunk's last timestep reads its own row again: xs has CH rows.
        float4 xnx = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (PIPE) xnx = *(const float4*)xs[jj + 1 < cn ? jj + 1 : jj];
        (void)xnx;
        float acc[DOUT];
#pragma unroll
        for (int r = 0; r < DOUT; ++r) acc[r] = accg[r].x + accg[r].y;
        if constexpr (DOUT >= 4) {
          const auto p01 = __builtin_amdgcn_permlane32_swap(f_bits(acc[0]), f_bits(acc[1]), false, false);
          const auto p23 = __builtin_amdgcn_permlane32_swap(f_bits(acc[2]), f_bits(acc[3]), false, false);
          const float s01 = bits_f(p01[0]) + bits_f(p01[1]);       // lanes 0..31: value 0, 32..63: value 1
          const float s23 = bits_f(p23[0]) + bits_f(p23[1]);
          const auto q = __builtin_amdgcn_permlane16_swap(f_bits(s01), f_bits(s23), false, false);
          float t4 = bits_f(q[0]) + bits_f(q[1]);                  // rows: values 0, 2, 1, 3
          t4 = row_sum_dpp(t4);
          if constexpr (DOUT == 5) {
            const float w4 = wave_sum_dpp(acc[4]);                 // lane 63
            if (wslot >= 0) red[par][wslot] = lane == 63 ? w4 : t4;
          } else {
            if (wslot >= 0) red[par][wslot] = t4;
          }
        } else {
          wave_sum_dpp_n<DOUT>(acc);
          if (lane == 63) {
#pragma unroll
            for (int r = 0; r < DOUT; ++r) red[par][r * 16 + wave] = acc[r];
          }
        }
        if constexpr (HA > 0) {
          // hoisted state halves, first place: behind the publication, in front of the barrier (delays the wave's arrival: few)
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int g = HD; g < HD + HA; ++g) hoist_state(g);
          __builtin_amdgcn_sched_barrier(0);
        }
        SSN_BSTAMP(bt3);
        __syncthreads();
        SSN_BSTAMP(bt4);
        if constexpr (PIPE) {
          const float rv = red[par][lane];
          float rv1 = 0.0f;
          if constexpr (DOUT > 4) rv1 = red[par][64 + lane];
          if constexpr (HB > 0) {
            // second place: between the LDS read of the wave sums and the wait for it - both waves of a SIMD fill it together
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = HD + HA; g < HT; ++g) hoist_state(g);
            __builtin_amdgcn_sched_barrier(0);
          }
          v0 = row_sum_dpp(rv);                                    // row r of every wave: total of decoded row r
          if constexpr (DOUT > 4) v1 = rv1;
        } else {
          v0 = row_sum_dpp(red[par][lane]);                        // row r of every wave: total of decoded row r
        }
        SSN_BSTAMP(bt5);
        if constexpr (SPLIT != 0) {
          if (P > 1) {
            // Split ensemble: the members publish their four sums and read their partners' (tools/xcd_exchange.hip measured
            // this protocol: +0.5 - 0.6 us per timestep wherever the members sit).  Three rotating buffers of sentinel
            // words: step t publishes into buffer t % 3 and resets the member's own words of buffer (t + 1) % 3, which
            // its partners read for the last time at step t - 2 (a partner that has published step t - 1 has consumed
            // everybody's step t - 2); the reset is acknowledged (s_waitcnt vmcnt(0)) before this step's publication.
            // Row r of every wave sums the members in lane order: identical totals, bit for bit, in every member.
            const int tq = j0 + jj;
            unsigned int* const xb = a.xslots + (size_t)k * 64;                      // [16 members][4 words] of one buffer
            const size_t bstride = (size_t)a.K * 64;
            if (wave == 0 && (lane & 15) == 0) {
              unsigned int* const pub = xb + (size_t)(tq % 3) * bstride + member * 4 + (lane >> 4);
              const unsigned int val = f_bits(v0);
              // (the reset of buffer (t + 1) % 3 was issued at the top of the timestep: its acknowledgement has arrived long ago)
              asm volatile("s_waitcnt vmcnt(0)\n\tglobal_store_dword %0, %1, off sc0 sc1" :: "v"(pub), "v"(val) : "memory");
            }
            const unsigned int* const src = xb + (size_t)(tq % 3) * bstride + (lane & 15) * 4 + (lane >> 4);
            const bool mine = (lane & 15) < P;
            unsigned int got = 0, spins = 0;
            while (true) {
              if (mine) asm volatile("global_load_dword %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(got) : "v"(src) : "memory");
              if (!__any(mine && got == BLOCK_XCHG_SENTINEL)) break;
              if (++spins > (1u << 20)) { if (lane == 0) *a.xerr = 1; break; }        // (a partner that never comes: no hang)
            }
            v0 = row_sum_dpp(mine ? bits_f(got) : 0.0f);
          }
        }
        F0 = __builtin_fmaf(la0, F0, lb0 * v0);                    // rows without a filter: la = lb = 0
        if constexpr (HD > 0) {
          // third place: between the filter update and the v_readlane that reads it
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int g = 0; g < HD; ++g) hoist_state(g);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (DOUT > 4) {
          if constexpr (PIPE) v1 = row_sum_dpp(v1); else v1 = row_sum_dpp(red[par][64 + lane]);
          F1 = __builtin_fmaf(la1, F1, lb1 * v1);
        }
        // pipelined: the next timestep's input first, the hand-off to the post stage behind it (the row was read in front of the
        // wave reduction: no LDS operation between the totals and the first encode FMA)
        if constexpr (PIPE) assemble_x(xnx);
        if (wave == 0 && member == 0) {
          if ((lane & 15) == 0 && (lane >> 4) < DOUT) os[jj][lane >> 4] = v0;
          if (DOUT > 4 && lane == 0) os[jj][4] = v1;
        }
        SSN_BSTAMP(bt6);
        SSN_BSTAMP_ADD(0, bt0, bt1); SSN_BSTAMP_ADD(1, bt1, bt2); SSN_BSTAMP_ADD(2, bt2, bt3); SSN_BSTAMP_ADD(3, bt3, bt4);
        SSN_BSTAMP_ADD(4, bt4, bt6); SSN_BSTAMP_ADD(5, bt4, bt5);
      } else {
        T acc[DOUT];
#pragma unroll
        for (int r = 0; r < DOUT; ++r) acc[r] = accg[r];
        wave_sum_dpp_n<DOUT>(acc);
        if (lane == 63) {
#pragma unroll
          for (int r = 0; r < DOUT; ++r) red[par][r * 16 + wave] = acc[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < DOUT; ++r) {
          T t = T(0);
#pragma unroll
          for (int w = 0; w < 16; ++w) t += red[par][r * 16 + w];
          tot[r] = t;
        }
#pragma unroll
        for (int r = 0; r < DOUT; ++r) fs[r] = la[r] * fs[r] + lb[r] * tot[r];    // rows without a filter: la = lb = 0
        if (tid < DOUT) {
          T v = T(0);
#pragma unroll
          for (int r = 0; r < DOUT; ++r) v = tid == r ? tot[r] : v;
          os[jj][tid] = v;
        }
      }
    }
  }
#ifdef SSN_BLOCK_STAMPS
  if constexpr (F32) {
    unsigned long long bm1, br1;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(bm1), "=s"(br1) :: "memory");
    if (lane == 0) {
      for (int i = 0; i < 5; ++i) atomicAdd(&g_block_stamps[i], bst[i]);
      atomicAdd(&g_block_stamps[8], bst[5]);
      atomicAdd(&g_block_stamps[5], (unsigned long long)a.B);
      if (k == 0 && wave == 0) { atomicAdd(&g_block_stamps[6], bm1 - bm0); atomicAdd(&g_block_stamps[7], br1 - br0); }
    }
  }
#endif
  if constexpr (F32 && SSN_BLOCK_SKIP != 0) {
    if (lane == 0 && a.slot_stats) {
      atomicAdd(a.slot_stats, (unsigned long long)n_slots);
      atomicAdd(a.slot_stats + 1, (unsigned long long)n_silent);
    }
  }
  __syncthreads();
  if (member == 0) {                         // last chunk's decoded rows
    const int j0 = (a.B - 1) / CH * CH, cn = a.B - j0;
    for (int i = tid; i < cn * DOUT; i += nthr) {
      const int jj = i / DOUT, r = i - jj * DOUT;
      if (s_out[r]) a.bsig[(size_t)(a.row0 + j0 + jj) * a.n_sig + s_dst[r]] = os[jj][r];
    }
  }

  // ---- state back to HBM; decoded values and filter states of the last step to the signal vector ------------
  int tid2 = tid;
  asm volatile("" : "+v"(tid2));      // fresh addresses: keeps NPT pointers from staying live across the time loop
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int i0 = (g * nthr + tid2) * PK;
    if constexpr (F32) s[g] = (f32x2){lif_word_out(s[g].x, lcRkq, lcTau), lif_word_out(s[g].y, lcRkq, lcTau)};
    if (i0 < n_loc) *reinterpret_cast<G*>(Sp + i0) = s[g];         // (padding elements of the row are never read back)
  }
  if constexpr (TAP != 0) {
    // the last timestep's tap values also go to the signal vector, like the decoded values below: every thread copies what it
    // wrote itself to the launch's last row
    if (tcol && a.B > 0) {
      const T* const lrow = a.bsig + (size_t)(a.row0 + a.B - 1) * a.n_sig;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int i0 = (g * nthr + tid2) * PK;
        if (i0 >= n_loc) continue;
#pragma unroll
        for (int c = 0; c < PK; ++c) {
          const int d = tcol[i0 + c];
          if (d >= 0) a.sig_w[d] = lrow[d];
        }
      }
    }
  }
  if (a.B > 0 && member == 0) {
    if constexpr (F32) {
      if (wave == 0 && (lane & 15) == 0 && (lane >> 4) < DOUT) {
        const int r = lane >> 4;
        a.sig_w[s_dst[r]] = v0;
        const int st = a.lp_state[(long long)k * DOUT + r];
        if (st >= 0) a.sig_w[st] = F0;
      }
      if (DOUT > 4 && tid == 0) {
        a.sig_w[s_dst[4]] = v1;
        const int st = a.lp_state[(long long)k * DOUT + 4];
        if (st >= 0) a.sig_w[st] = F1;
      }
    } else if (tid < DOUT) {
      T v = T(0), f = T(0);
#pragma unroll
      for (int r = 0; r < DOUT; ++r) { v = tid == r ? tot[r] : v; f = tid == r ? fs[r] : f; }
      a.sig_w[s_dst[tid]] = v;
      const int st = a.lp_state[(long long)k * DOUT + tid];
      if (st >= 0) a.sig_w[st] = f;
    }
  }
}

constexpr int BLOCK_LDS_BYTES = 160 * 1024, BLOCK_STATIC_LDS = 2560;     // CU capacity; bound on the kernel's static arrays

template <typename T, int DIN, int DOUT, int NPT, int TPB, int LDSW, int SPLIT, int TAP = 0>
static hipError_t launch_block_variant_s(hipStream_t s, const BlockArgs<T>& a) {
  const int lds = LDSW * a.threads * NPT * (int)sizeof(T);
  static std::atomic<uint64_t> configured{0};
  if (LDSW > 0) {
    hipError_t e = set_max_dynamic_lds_once(reinterpret_cast<const void*>(&k_ens_block<T, DIN, DOUT, NPT, TPB, LDSW, SPLIT, TAP>),
                                            BLOCK_LDS_BYTES - BLOCK_STATIC_LDS, configured);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_ens_block<T, DIN, DOUT, NPT, TPB, LDSW, SPLIT, TAP>), dim3((unsigned)(a.K * (SPLIT ? a.P : 1))), dim3((unsigned)a.threads), lds, s, a);
  return hipGetLastError();
}
template <typename T, int DIN, int DOUT, int NPT, int TPB, int LDSW>
static hipError_t launch_block_variant(hipStream_t s, const BlockArgs<T>& a) {
  if (a.P > 1) {
    if constexpr (sizeof(T) == 4 && DOUT <= 4) return launch_block_variant_s<T, DIN, DOUT, NPT, TPB, LDSW, 1>(s, a);
    else return hipErrorInvalidValue;
  }
  if (a.tap_slot) {      // the tapped twin (never a silent drop: a build whose time loop leaves slots out has none)
    if constexpr (SSN_BLOCK_SKIP == 0) return launch_block_variant_s<T, DIN, DOUT, NPT, TPB, LDSW, 0, 1>(s, a);
    else return hipErrorInvalidValue;
  }
  return launch_block_variant_s<T, DIN, DOUT, NPT, TPB, LDSW, 0>(s, a);
}

// (workgroup size, neurons per thread, parameter rows in LDS) variants, in the order the planner tries them.  A wave's
// register budget is 512 / (waves per SIMD): 1024 threads -> 128, 768 -> 168, 512 -> 256; a neuron keeps
// din + dout + 2 words (9 at din 3, dout 4) of which the LDS rows take 3.  Measured on MI355X at n = 10 000
// (tools/bench_block.py, profiles/round2_block_variants.txt): (512, 20, LDS) 3.49 ms per 1000 timesteps of config 2,
// (768, 14, LDS) 3.68 - more waves per SIMD do not pay: every wave repeats the per-timestep reductions.
struct BlockVariant { int tpb, npt, ldsw; };
template <typename T> struct BlockVariants;
template <> struct BlockVariants<float> {
  static constexpr int N = 7;
  static constexpr BlockVariant v[N] = {{1024, 2, 0}, {1024, 4, 0}, {512, 6, 0}, {1024, 6, 0}, {512, 10, 0}, {512, 20, 3}, {768, 14, 3}};
};
template <> struct BlockVariants<double> {
  static constexpr int N = 3;
  static constexpr BlockVariant v[N] = {{1024, 1, 0}, {1024, 2, 0}, {1024, 4, 0}};
};

template <typename T, int DIN, int DOUT>
static hipError_t launch_block_npt(hipStream_t s, const BlockArgs<T>& a) {
  const int key = (a.tpb * 100 + a.npt) * 8 + a.enc_lds;
  switch (key) {
#define SSN_CASE(TPB, N, L) case (TPB * 100 + N) * 8 + L: return launch_block_variant<T, DIN, DOUT, N, TPB, L>(s, a);
    SSN_CASE(1024, 2, 0) SSN_CASE(1024, 4, 0)
#undef SSN_CASE
#define SSN_CASE(TPB, N, L) case (TPB * 100 + N) * 8 + L: if constexpr (sizeof(T) == 8) return launch_block_variant<T, DIN, DOUT, N, TPB, L>(s, a); else return hipErrorInvalidValue;
    SSN_CASE(1024, 1, 0)
#undef SSN_CASE
#define SSN_CASE(TPB, N, L) case (TPB * 100 + N) * 8 + L: if constexpr (sizeof(T) == 4) return launch_block_variant<T, DIN, DOUT, N, TPB, L>(s, a); else return hipErrorInvalidValue;
    SSN_CASE(1024, 6, 0) SSN_CASE(512, 6, 0) SSN_CASE(512, 10, 0) SSN_CASE(512, 20, 3) SSN_CASE(768, 14, 3)
#undef SSN_CASE
    default: return hipErrorInvalidValue;
  }
}

template <typename T>
bool ens_block_supported(int din, int dout, int n, const int want[3], int* threads, int* tpb, int* npt, int* enc_lds) {
  if (!(din == 3 && dout >= 3 && dout <= 5)) return false;
  const int want_tpb = want[0], want_npt = want[1], want_lds = want[2];      // tuning knob SSN_BLOCK_VARIANT (all 0: the first variant that fits)
  const int pk = sizeof(T) == 4 ? 2 : 1;         // neurons per group; single-group variants run n / pk threads
  for (int i = 0; i < BlockVariants<T>::N; ++i) {
    const BlockVariant v = BlockVariants<T>::v[i];
    if (want_tpb && (v.tpb != want_tpb || v.npt != want_npt || v.ldsw != want_lds)) continue;
    int th = v.tpb;
    if (v.npt == pk && n < th * pk) th = std::max(64, ((n + pk - 1) / pk + 63) / 64 * 64);
    if ((int64_t)th * v.npt < n) continue;
    if ((int64_t)v.ldsw * th * v.npt * (int64_t)sizeof(T) > BLOCK_LDS_BYTES - BLOCK_STATIC_LDS) continue;
    *threads = th; *tpb = v.tpb; *npt = v.npt; *enc_lds = v.ldsw;
    return true;
  }
  return false;
}

template <typename T>
hipError_t launch_ens_block(hipStream_t s, const BlockArgs<T>& a) {
  if (a.din == 3 && a.dout == 5) return launch_block_npt<T, 3, 5>(s, a);
  if (a.din == 3 && a.dout == 4) return launch_block_npt<T, 3, 4>(s, a);
  if (a.din == 3 && a.dout == 3) return launch_block_npt<T, 3, 3>(s, a);
  return hipErrorInvalidValue;
}

}  // namespace ssn
