// ssn_micro_kinds.hpp - what a micro-operator kind is: its number (MicroKind) and what kernels and planner ask about it
// (micro_row_kind, MICRO_KINDS).  Plain C++17, no HIP: kernels, host executor and the CPU-side planners share it.
#pragma once

namespace ssn {

enum MicroKind {
  M_FILL = 1, M_AXPY_INC, M_AXPY_SET, M_LOWPASS, M_TABLE, M_MATVEC_INC, M_MATVEC_SET, M_ENS_FINISH,
  M_GATE, M_ARGMAX_GATHER, M_PROBE, M_STEP_END, M_ROW_IN, M_ROW_OUT, M_REDUCE_SET, M_REDUCE_INC,
  M_LINCOMB            // dst = a * dst + b * (c + sum_k alpha_k * sig[src_k + i]); p0 = LinTerm[i0]
};
// Row kinds: one thread computes one output row (micro_row, ssn_micro.hpp), so a block of the round kernel takes GLUE_ROWS rows
// of them where it takes GLUE_CHUNK elements of an element-wise kind.  Kernels and planner (MK_GLUE_ROW) both ask here.
constexpr bool micro_row_kind(int kind) {
  return kind == M_MATVEC_INC || kind == M_MATVEC_SET || kind == M_ENS_FINISH || kind == M_REDUCE_SET || kind == M_REDUCE_INC;
}

// What the planner asks about a micro-operator kind (ssn::MicroKind): one row per kind, one flag per question.  What a kind
// reads and writes is Sim::micro_access; every "is it one of these kinds" is a lookup here.
enum MicroKindFlag {
  MK_SAME_THREAD = 1,   // element-wise in a program, element p of a range on thread (p - origin) mod 1024: follows an operator it depends on
                        // without a barrier when their origins agree (push_micro); a glue member of a serial chain (solo_lat)
  MK_VECOPS = 2,        // may move into the grid-wide head of the item plan (k_vecops)
  MK_CUT = 4,           // cut at the range endpoints of the other operators (split_micro)
  MK_CHAIN = 8,         // may join a chain of element-aligned operators (chainable)
  MK_GLUE_ROW = 16,     // a glue block takes GLUE_ROWS rows of it, not GLUE_CHUNK elements (emit)
  MK_BATCH_EW = 32,     // time-batched stage: element-wise, shares a launch with its neighbours (stage::hazard, stage::pack)
  MK_BATCH_R = 64,      // time-batched stage: reads src
  MK_BATCH_W = 128,     // time-batched stage: writes dst
  MK_BATCH_PRODUCT = 256 // time-batched stage: a matrix product - reads `cols` elements of src, not `len` (stage::batch_read_len, ZeroMap)
};
// A kind appended to ssn::MicroKind takes: the enum above, one `case` in ssn_micro.hpp (what it computes - every kernel that
// runs micro-operators calls that one definition), its row below (without one it would read as "no flags") and its row in
// Sim::micro_access (ssn_host.hip: what it reads and writes).
static_assert(M_LINCOMB == 17, "MICRO_KINDS has a row for every MicroKind up to M_LINCOMB: add the new kind's");
struct MicroKindTable {
  unsigned short f[M_LINCOMB + 1] = {};
  constexpr MicroKindTable() {
    f[M_FILL] = MK_SAME_THREAD | MK_VECOPS | MK_CUT | MK_CHAIN | MK_BATCH_EW | MK_BATCH_W;
    f[M_AXPY_INC] = f[M_AXPY_SET] = MK_SAME_THREAD | MK_VECOPS | MK_CUT | MK_CHAIN | MK_BATCH_EW | MK_BATCH_R | MK_BATCH_W;
    f[M_LOWPASS] = MK_SAME_THREAD | MK_VECOPS | MK_CUT | MK_CHAIN | MK_BATCH_R | MK_BATCH_W;
    f[M_TABLE] = MK_SAME_THREAD | MK_VECOPS | MK_CHAIN | MK_BATCH_EW | MK_BATCH_W;
    f[M_ROW_IN] = MK_SAME_THREAD | MK_VECOPS | MK_CUT | MK_CHAIN;
    f[M_ROW_OUT] = MK_SAME_THREAD | MK_CUT | MK_CHAIN;
    f[M_PROBE] = MK_SAME_THREAD | MK_CHAIN | MK_BATCH_EW | MK_BATCH_R;
    f[M_LINCOMB] = MK_CUT | MK_CHAIN;
    f[M_REDUCE_SET] = f[M_REDUCE_INC] = MK_CHAIN | MK_GLUE_ROW;
    f[M_MATVEC_INC] = f[M_MATVEC_SET] = MK_GLUE_ROW | MK_BATCH_R | MK_BATCH_W | MK_BATCH_PRODUCT;
    f[M_ENS_FINISH] = MK_GLUE_ROW;
    // M_GATE, M_ARGMAX_GATHER, M_STEP_END: none
  }
};
constexpr MicroKindTable MICRO_KINDS;
constexpr bool kind_is(int kind, int flag) { return kind > 0 && kind <= M_LINCOMB && (MICRO_KINDS.f[kind] & flag) != 0; }
// (the round kernel chunks an operator by ssn::micro_row_kind, the planner counts its blocks by MK_GLUE_ROW)
constexpr bool glue_rows_agree() {
  for (int k = 0; k <= M_LINCOMB + 1; ++k) if (kind_is(k, MK_GLUE_ROW) != micro_row_kind(k)) return false;
  return true;
}
static_assert(glue_rows_agree(), "MK_GLUE_ROW and ssn::micro_row_kind name different kinds");

}  // namespace ssn
