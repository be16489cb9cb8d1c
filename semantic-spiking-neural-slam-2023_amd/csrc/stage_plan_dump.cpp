// stage_plan_dump.cpp - the planner of ssn_stage_plan.hpp on a CPU, as text (tests/test_stage_plan.py).  Not part of the library:
//   c++ -std=c++17 -O2 stage_plan_dump.cpp -o stage_plan_dump
// An operator is one line `kind dst src len cols prev a gain`; the coefficients are doubles, narrowed as plan() narrows them:
// a = (T)a, b = (T)((1 - a) * gain).  Every subcommand reads stdin; a line `end` closes a list, and the answer to it ends with `end`.
//   stage_plan_dump kinds                             <number> <name> [ew] [r] [w] [product] per MicroKind (the MK_BATCH_* flags)
//   stage_plan_dump plan f32|f64 [no-stage-batch]     per list: the optimised operators as SSN_DEBUG_PLAN lists them, then
//                                                     `launch <first> <count>` per launch
//   stage_plan_dump zero f32|f64                      per list: operators, a line `blocks`, then per block one line of 0 | 1 for each
//       M_TABLE operator in list order (1: its table is zero in that block); answer per block, over the optimised operators:
//       `block <n> skipped <index>... set <index>...` (products left out; those among them whose rows are marked zero)
//   stage_plan_dump dispatch                          lines `kind len cols B f32|f64` -> the kernel's name (`nothing`: no launch)
//   stage_plan_dump hazard                            two operator lines per pair (the earlier one first) -> 0 | 1 | 2
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "ssn_stage_plan.hpp"
namespace stage = ssn::stage;

static int usage() {
  std::fprintf(stderr, "usage: stage_plan_dump kinds | plan f32|f64 [no-stage-batch] | zero f32|f64 | dispatch | hazard   (input on stdin)\n");
  return 2;
}

static int kinds() {
  const char* names[ssn::M_LINCOMB + 1] = {};
#define NAME(k) names[ssn::k] = #k
  NAME(M_FILL); NAME(M_AXPY_INC); NAME(M_AXPY_SET); NAME(M_LOWPASS); NAME(M_TABLE); NAME(M_MATVEC_INC); NAME(M_MATVEC_SET); NAME(M_ENS_FINISH);
  NAME(M_GATE); NAME(M_ARGMAX_GATHER); NAME(M_PROBE); NAME(M_STEP_END); NAME(M_ROW_IN); NAME(M_ROW_OUT); NAME(M_REDUCE_SET); NAME(M_REDUCE_INC);
  NAME(M_LINCOMB);
#undef NAME
  for (int k = 1; k <= ssn::M_LINCOMB; ++k)
    std::printf("%d %s%s%s%s%s\n", k, names[k] ? names[k] : "?", ssn::kind_is(k, ssn::MK_BATCH_EW) ? " ew" : "", ssn::kind_is(k, ssn::MK_BATCH_R) ? " r" : "",
                ssn::kind_is(k, ssn::MK_BATCH_W) ? " w" : "", ssn::kind_is(k, ssn::MK_BATCH_PRODUCT) ? " product" : "");
  return 0;
}

template <typename T>
static bool parse_op(const std::string& line, ssn::BatchOp<T>* o) {
  double a = 0, gain = 0;
  *o = ssn::BatchOp<T>{};
  if (std::sscanf(line.c_str(), "%d %lld %lld %lld %d %d %lf %lf", &o->kind, &o->dst, &o->src, &o->len, &o->cols, &o->src_prev, &a, &gain) != 8) return false;
  o->a = (T)a;
  o->b = (T)((1.0 - a) * gain);
  return o->dst >= 0 && o->src >= 0 && o->len >= 0 && o->cols >= 0;
}

// One list of `plan` / `zero`.  The tables' zero flags travel as Sim's table ids do: p0 points at the operator's slot.
template <typename T>
static int one_list(const std::vector<ssn::BatchOp<T>>& read, const std::vector<std::vector<char>>& blocks, bool zero, bool stage_batch) {
  std::vector<ssn::BatchOp<T>> ops = read;
  std::vector<char> slots(ops.size() + 1, 0);
  size_t n_tables = 0;
  long long n_sig = 0;
  for (ssn::BatchOp<T>& o : ops) {
    if (o.kind == ssn::M_TABLE) o.p0 = &slots[n_tables++];
    n_sig = std::max({n_sig, o.dst + o.len, o.src + stage::batch_read_len(o)});
  }
  ops = stage::optimise(ops);
  if (!zero) {
    for (const ssn::BatchOp<T>& o : ops) std::printf("[ssn]   batch op kind %d dst %lld src %lld len %lld cols %d prev %d\n", o.kind, (long long)o.dst, (long long)o.src, (long long)o.len, o.cols, o.src_prev);
    for (const stage::Launch& l : stage::pack(ops, stage_batch)) std::printf("launch %d %d\n", l.first, l.count);
    return 0;
  }
  const std::vector<stage::Launch> launches = stage::pack(ops, true);
  for (size_t n = 0; n < blocks.size(); ++n) {
    if (blocks[n].size() != n_tables) return usage();
    stage::ZeroMap<T> zeros(n_sig, true);
    auto note = [&](const ssn::BatchOp<T>& o) { zeros.note(o, o.kind == ssn::M_TABLE && blocks[n][(size_t)((const char*)o.p0 - slots.data())] != 0); };
    std::string skipped, set;
    for (const stage::Launch& l : launches) {          // the walk of Sim::run_batch (ssn_host.hip) without the launches
      const ssn::BatchOp<T>& o = ops[(size_t)l.first];
      if (l.count > 1) {
        for (int q = 0; q < l.count; ++q) note(ops[(size_t)(l.first + q)]);
      } else if (zeros.skippable(o)) {
        skipped += " " + std::to_string(l.first);
        if (o.kind == ssn::M_MATVEC_SET) set += " " + std::to_string(l.first);
        zeros.note_skipped(o);
      } else {
        note(o);
      }
    }
    std::printf("block %zu skipped%s set%s\n", n, skipped.c_str(), set.c_str());
  }
  return 0;
}

template <typename T>
static int lists(bool zero, bool stage_batch) {
  std::vector<ssn::BatchOp<T>> ops;
  std::vector<std::vector<char>> blocks;
  bool in_blocks = false;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line == "end") {
      if (one_list<T>(ops, blocks, zero, stage_batch)) return 2;
      std::printf("end\n");
      ops.clear(); blocks.clear(); in_blocks = false;
    } else if (zero && line == "blocks") {
      in_blocks = true;
    } else if (in_blocks) {
      std::vector<char> flags;
      std::istringstream in(line);
      for (int v; in >> v;) flags.push_back(v != 0);
      blocks.push_back(flags);
    } else {
      ssn::BatchOp<T> o;
      if (!parse_op<T>(line, &o)) return usage();
      ops.push_back(o);
    }
  }
  return ops.empty() && blocks.empty() ? 0 : usage();      // (a list without its `end`)
}

static int dispatch() {
  static const char* const NAMES[] = {"nothing", "kb_lowpass", "kb_lowpass_chunked", "kb_gemm", "kb_gemm_mfma_f32", "kb_elementwise"};
  static_assert(stage::KB_NOTHING == 0 && stage::KB_LOWPASS == 1 && stage::KB_LOWPASS_CHUNKED == 2 && stage::KB_GEMM == 3 && stage::KB_GEMM_MFMA_F32 == 4 &&
                stage::KB_ELEMENTWISE == 5, "NAMES is indexed by stage::Kernel");
  std::string line;
  while (std::getline(std::cin, line)) {
    int kind = 0, cols = 0, B = 0;
    long long len = 0;
    char dtype[8] = "";
    if (std::sscanf(line.c_str(), "%d %lld %d %d %7s", &kind, &len, &cols, &B, dtype) != 5 || (std::strcmp(dtype, "f32") && std::strcmp(dtype, "f64"))) return usage();
    std::printf("%s\n", NAMES[stage::kernel_for(kind, len, cols, B, !std::strcmp(dtype, "f32"))]);
  }
  return 0;
}

static int hazards() {
  std::string first, second;
  while (std::getline(std::cin, first)) {
    ssn::BatchOp<double> a, b;
    if (!std::getline(std::cin, second) || !parse_op<double>(first, &a) || !parse_op<double>(second, &b)) return usage();
    std::printf("%d\n", stage::hazard(a, b));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "kinds")) return kinds();
  if (argc == 2 && !std::strcmp(argv[1], "dispatch")) return dispatch();
  if (argc == 2 && !std::strcmp(argv[1], "hazard")) return hazards();
  const bool plan = argc >= 3 && !std::strcmp(argv[1], "plan"), zero = argc == 3 && !std::strcmp(argv[1], "zero");
  const bool no_batch = plan && argc == 4 && !std::strcmp(argv[3], "no-stage-batch");
  if (!(zero || (plan && (argc == 3 || no_batch)))) return usage();
  if (!std::strcmp(argv[2], "f32")) return lists<float>(zero, !no_batch);
  if (!std::strcmp(argv[2], "f64")) return lists<double>(zero, !no_batch);
  return usage();
}
