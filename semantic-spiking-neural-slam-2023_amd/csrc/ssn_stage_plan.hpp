// ssn_stage_plan.hpp - the planner of the time-batched stages: what two operators of a stage do to each other (hazard), the
// order they run in (optimise), the launches they share (pack), which products multiply nothing but zeros (ZeroMap) and the
// kernel an operator goes to (kernel_for).  Plain C++17, no HIP, no environment, no output: Sim (ssn_host.hip) and
// launch_batch_op (ssn_kernels.hpp) call it on the GPU side, stage_plan_dump.cpp prints it on a CPU (tests/test_stage_plan.py).
#pragma once
#include <algorithm>
#include <vector>
#include "ssn_micro_kinds.hpp"

namespace ssn {

// One operator of a time-batched stage, executed for rows t = 0..B-1 of the block.  Row r of the block
// buffer `bsig` ([B+1][n_sig]) holds the signals after step (block_start + r); row 0 is the carry-in.
// (BatchOp and BatchOpList are kernel arguments: they stay in namespace ssn, where the kernels' signatures name them.)
template <typename T>
struct BatchOp {
  T* bsig;
  long long n_sig;       // row stride
  int B;
  int kind;              // MicroKind (M_FILL, M_AXPY_*, M_LOWPASS, M_TABLE, M_MATVEC_*, M_PROBE)
  long long dst, src, len;   // len = rows for matvec
  int cols, ld;
  int src_prev;          // 1: read row t (value before this step's update) instead of row t+1
  T a, b;
  const void* p0;        // W | TableSlot* | ProbeSlot*
  long long step0;       // = block_start
};
constexpr int MAX_BATCH_OPS = 24;
template <typename T> struct BatchOpList { BatchOp<T> op[MAX_BATCH_OPS]; int count; };

namespace stage {

constexpr int MAX_CUT_OFFSETS = 32;    // a reset / sum whose range holds more cut offsets than this (its own two ends included) stays whole

// Element-wise operators of a time-batched stage: what they write / read (column ranges; rows are handled alike).
template <typename T> bool batch_elementwise(const BatchOp<T>& o) { return kind_is(o.kind, MK_BATCH_EW); }
template <typename T> bool batch_writes(const BatchOp<T>& o) { return kind_is(o.kind, MK_BATCH_W); }
template <typename T> bool batch_reads(const BatchOp<T>& o) { return kind_is(o.kind, MK_BATCH_R); }
template <typename T> long long batch_read_len(const BatchOp<T>& o) { return kind_is(o.kind, MK_BATCH_PRODUCT) ? o.cols : o.len; }
// Hazard between two operators of a stage, `a` the earlier one.  0: none; 1: only on elements that both touch at the SAME
// index of the same row (equal range origins, no previous-row read of what the other writes) - two element-wise operators
// may then share a launch, the same thread runs them in order (kb_elementwise_multi); 2: anything else.
template <typename T>
int hazard(const BatchOp<T>& a, const BatchOp<T>& b) {
  auto ov = [](long long x, long long xl, long long y, long long yl) { return x < y + yl && y < x + xl; };
  int kind = 0;
  auto pair = [&](long long x, long long xl, long long y, long long yl, bool prev) {
    if (!ov(x, xl, y, yl)) return;
    kind = std::max(kind, (x == y && !prev) ? 1 : 2);
  };
  if (batch_writes(a) && batch_writes(b)) pair(a.dst, a.len, b.dst, b.len, false);
  if (batch_writes(a) && batch_reads(b)) pair(a.dst, a.len, b.src, batch_read_len(b), b.src_prev != 0);
  if (batch_reads(a) && batch_writes(b)) pair(a.src, batch_read_len(a), b.dst, b.len, a.src_prev != 0);
  if (kind == 1 && !(batch_elementwise(a) && batch_elementwise(b))) kind = 2;
  return kind;
}

// Order of a time-batched stage: the builder hands its operators over in one valid order (stages.py `border`), in which
// independent operators of different kinds alternate (a scan, the sum that reads it, the next scan ...) and every one is
// a launch.  Here: resets and sums are cut at the range endpoints of the other operators (the reset of all accumulators
// of a network then lines up with each consumer), every operator takes the earliest dependency level its hazards allow,
// operators are sorted by level and kind, and neighbouring scans with equal coefficients over adjacent ranges are joined
// again.  pack then puts consecutive element-wise operators - also dependent ones, see hazard - into launches.
template <typename T>
std::vector<BatchOp<T>> optimise(const std::vector<BatchOp<T>>& ops) {
  typedef BatchOp<T> Op;
  std::vector<long long> cuts;
  for (const Op& o : ops) {
    if (batch_writes(o)) { cuts.push_back(o.dst); cuts.push_back(o.dst + o.len); }
    if (batch_reads(o)) { cuts.push_back(o.src); cuts.push_back(o.src + batch_read_len(o)); }
  }
  std::sort(cuts.begin(), cuts.end());
  cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
  std::vector<Op> cut;
  for (const Op& o : ops) {
    const bool axpy = o.kind == M_AXPY_INC || o.kind == M_AXPY_SET;
    if (!(axpy || o.kind == M_FILL) || o.len <= 1) { cut.push_back(o); continue; }
    std::vector<long long> offs{0, o.len};
    for (long long base : {o.dst, axpy ? o.src : o.dst}) {
      auto lo = std::upper_bound(cuts.begin(), cuts.end(), base), hi = std::lower_bound(cuts.begin(), cuts.end(), base + o.len);
      for (auto it = lo; it < hi; ++it) offs.push_back(*it - base);
    }
    std::sort(offs.begin(), offs.end());
    offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
    if (offs.size() > (size_t)MAX_CUT_OFFSETS) { cut.push_back(o); continue; }
    for (size_t q = 0; q + 1 < offs.size(); ++q) {
      Op pc = o;
      pc.dst = o.dst + offs[q]; pc.len = offs[q + 1] - offs[q];
      if (axpy) pc.src = o.src + offs[q];
      cut.push_back(pc);
    }
  }
  const size_t n = cut.size();
  std::vector<int> level(n, 0);
  for (size_t j = 0; j < n; ++j)
    for (size_t i = 0; i < j; ++i)
      if (hazard(cut[i], cut[j])) level[j] = std::max(level[j], level[i] + 1);
  auto cls = [](const Op& o) { return batch_elementwise(o) ? 0 : o.kind == M_LOWPASS ? 1 : 2; };
  std::vector<size_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
    if (level[x] != level[y]) return level[x] < level[y];
    if (cls(cut[x]) != cls(cut[y])) return cls(cut[x]) < cls(cut[y]);
    return cut[x].kind == M_LOWPASS && cut[y].kind == M_LOWPASS && cut[x].dst < cut[y].dst;
  });
  std::vector<Op> out;
  int last_level = -1;
  for (size_t k : order) {
    const Op& o = cut[k];
    if (!out.empty() && level[k] == last_level && o.kind == M_LOWPASS && out.back().kind == M_LOWPASS && out.back().a == o.a && out.back().b == o.b &&
        out.back().src_prev == o.src_prev && out.back().dst + out.back().len == o.dst && out.back().src + out.back().len == o.src) {
      out.back().len += o.len;
      continue;
    }
    out.push_back(o);
    last_level = level[k];
  }
  return out;
}

// The launches of a stage over its (optimised) operators [first, first + count).  count > 1: one kb_elementwise_multi launch -
// consecutive element-wise operators share one unless a hazard between them crosses threads (hazard == 2), at most MAX_BATCH_OPS
// of them.  count == 1: a launch of its own (launch_batch_op): everything else, a list of one, and every operator when
// `stage_batch` is false (SSN_PLAN_NO_STAGE_BATCH).  Nothing here changes from block to block.
struct Launch { int first, count; };
template <typename T>
std::vector<Launch> pack(const std::vector<BatchOp<T>>& ops, bool stage_batch) {
  std::vector<Launch> out;
  for (size_t i = 0; i < ops.size();) {
    size_t j = i + 1;
    if (stage_batch && batch_elementwise(ops[i]))
      for (; j < ops.size() && j - i < (size_t)MAX_BATCH_OPS && batch_elementwise(ops[j]); ++j) {
        bool clash = false;
        for (size_t q = i; q < j; ++q) clash = clash || hazard(ops[q], ops[j]) == 2;
        if (clash) break;
      }
    out.push_back({(int)i, (int)(j - i)});
    i = j;
  }
  return out;
}

// Signal elements known to be ZERO in every row of one block: a table without an entry for any timestep of the block
// (the init-SSP input of the path integrator after its first 50 ms, reference run_pathint.py:136), and what fills /
// copies / products make of zeros.  A product whose whole input is zero is not multiplied out (PathIntegration config 2:
// the 1000 x 1015 x 1524 to_Fourier GEMM of every block but the first - 47 of a block's 3480 us).  `track` false
// (SSN_NO_ZERO_SKIP): nothing is known, nothing is skippable.
template <typename T>
class ZeroMap {
 public:
  ZeroMap(long long n_sig, bool track) : zero_(track ? (size_t)n_sig : 0, 0), track_(track) {}
  // effect of an operator that IS executed; `table_is_zero`: an M_TABLE's table has no entry in this block
  void note(const BatchOp<T>& o, bool table_is_zero) {
    if (!track_) return;
    switch (o.kind) {
      case M_TABLE: set_zero(o.dst, o.len, table_is_zero); break;
      case M_FILL: set_zero(o.dst, o.len, o.a == T(0)); break;
      case M_AXPY_SET: set_zero(o.dst, o.len, !o.src_prev && all_zero(o.src, o.len)); break;
      case M_AXPY_INC: if (o.src_prev || !all_zero(o.src, o.len)) set_zero(o.dst, o.len, false); break;
      case M_PROBE: break;
      default: set_zero(o.dst, o.len, false); break;          // products, filters: not known
    }
  }
  // a product whose whole input is zero in this block (never one that reads the previous row: row 0 is the last block's)
  bool skippable(const BatchOp<T>& o) const { return track_ && kind_is(o.kind, MK_BATCH_PRODUCT) && !o.src_prev && all_zero(o.src, o.cols); }
  // effect of a skipped product.  W @ 0: the result rows of the block are zero (the caller clears them); an increment adds nothing
  void note_skipped(const BatchOp<T>& o) { if (o.kind == M_MATVEC_SET) set_zero(o.dst, o.len, true); }

 private:
  bool all_zero(long long lo, long long n) const { for (long long q = lo; q < lo + n; ++q) if (!zero_[(size_t)q]) return false; return n > 0; }
  void set_zero(long long lo, long long n, bool v) { for (long long q = lo; q < lo + n; ++q) zero_[(size_t)q] = v ? 1 : 0; }
  std::vector<char> zero_;
  bool track_;
};

// The kernel one operator of a block of B timesteps goes to (launch_batch_op switches on it).  f32 has the chunked scan from
// CHUNKED_SCAN_MIN_B timesteps and the matrix-core product from MFMA_MIN_COLS x MFMA_MIN_ROWS x MFMA_MIN_B; f64 has neither.
enum Kernel { KB_NOTHING, KB_LOWPASS, KB_LOWPASS_CHUNKED, KB_GEMM, KB_GEMM_MFMA_F32, KB_ELEMENTWISE };
constexpr int CHUNKED_SCAN_MIN_B = 256, MFMA_MIN_COLS = 64, MFMA_MIN_ROWS = 32, MFMA_MIN_B = 32;
constexpr Kernel kernel_for(int kind, long long len, int cols, int B, bool f32) {
  if (B <= 0 || len <= 0) return KB_NOTHING;
  if (kind == M_LOWPASS) return f32 && B >= CHUNKED_SCAN_MIN_B ? KB_LOWPASS_CHUNKED : KB_LOWPASS;
  if (kind == M_MATVEC_INC || kind == M_MATVEC_SET) return f32 && cols >= MFMA_MIN_COLS && len >= MFMA_MIN_ROWS && B >= MFMA_MIN_B ? KB_GEMM_MFMA_F32 : KB_GEMM;
  return KB_ELEMENTWISE;
}

}  // namespace stage
}  // namespace ssn
