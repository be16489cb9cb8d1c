// ssn_host.hip - C ABI (include/ssn.h) and step-loop executor of libssn_hip.so.
//
// ssn_create turns the host-built operator list into a launch plan:
//   * runs of small vector operators become "programs" (one k_program launch each),
//   * ensemble arrays, dense matvecs, neuron updates and learning rules become their own kernels,
//   * the tail program of step s and the head program of step s+1 are fused into one launch,
//   * `steps_per_graph` consecutive timesteps are captured into one hipGraph; ssn_run_steps
//     replays it, so the host issues one graph launch per `steps_per_graph` simulated steps.
// Every kernel reads the current step from device memory (StepCtx), which is what makes the
// captured graph step-invariant.  There is no CPU fallback: without a HIP device ssn_create fails.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ssn.h"
#include "ssn_launch.hpp"
#include "ssn_fft_plan.hpp"
#include "ssn_recall.hpp"

namespace {

__global__ void k_set_block(ssn::StepCtx* ctx, long long block_start) { ctx->block_start = block_start; }
__global__ void k_advance(ssn::StepCtx* ctx, long long n) { ctx->step += n; }

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

}  // namespace
namespace ssn {
int probe_fail(int code, const char* what, hipError_t e) {
  return e == hipSuccess ? fail(code, "%s", what) : fail(code, "%s failed: %s", what, hipGetErrorString(e));
}
}  // namespace ssn
namespace {

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e__ = (expr);                                                                      \
    if (e__ != hipSuccess)                                                                        \
      return fail(e__ == hipErrorOutOfMemory ? SSN_ENOMEM : SSN_EHIP, "%s failed: %s (%s:%d)",    \
                  #expr, hipGetErrorString(e__), __FILE__, __LINE__);                             \
  } while (0)

#define CHK(expr)                     \
  do {                                \
    int rc__ = (expr);                \
    if (rc__ != SSN_OK) return rc__;  \
  } while (0)

struct Buf {
  void* d = nullptr;
  int64_t count = 0;
  int kind = 0;
  int64_t rows = 1, cols = 0, ld = 0;     // device layout (row padded)
  bool shaped = false;
  bool keep = false;                      // keep host copy for reset (state / learned)
  std::vector<double> host;               // initial contents if keep
  // ensemble-array fast path (k_ensarray FAST): decoders neuron-major, (V, R) packed into the V buffer
  int dec_K = 0, dec_dout = 0, dec_n = 0, dec_DP = 0;   // dec_DP > 0: stored [K][ld][DP] instead of [K*dout][ld]
  int packed = 0;                         // 1: holds packed LIF state words; 2: refractory view of buffer `partner`
  int partner = -1;
  // spike-sparse decoders (k_spmv_partial): logical [rows][cols] stored neuron-major [cols][ldt]
  bool transposed = false;
  int64_t ldt = 0;
  // neuron order on the device (whole-block kernel, Sim::reorder_block_neurons): column c of the rows of ensemble k holds the
  // neuron perm[k * cols + c] of the caller's order; perm_rows = rows per ensemble.  Empty: the caller's order.
  std::shared_ptr<std::vector<int32_t>> perm;
  int perm_rows = 1;
};

enum ItemType { IT_PROGRAM = 0, IT_ENS, IT_MATVEC, IT_NEURONS, IT_PES, IT_VOJA, IT_MATVEC_ORDERED, IT_FINISH, IT_SPMV, IT_DFT, IT_VECOPS, IT_GRID_LHS, IT_GRID_GEMM, IT_ARGMAX_PART, IT_ROUND,
                IT_GRID_DOT,        // (a body of the round grid only)
                IT_MATVEC_NEURONS,  // (round plan) a dense population's encoder product with the neuron update in its epilogue
                IT_NONE };          // (round plan) an operator that was folded into another one

// What the planner asks about a micro-operator kind - ssn::kind_is(kind, ssn::MK_*) - is one table in ssn_micro_kinds.hpp.
using ssn::kind_is;

// Plan options: ssn_model_desc.flags and the environment knobs, read once at ssn_create and constant for the simulator's
// life.  PlanOptions::read is the only caller of getenv in the library.  One row per knob: how the variable is read, the
// member, the variable, the default, the meaning ("Environment switches", lists the same rows).
//   PRESENT  true when the variable is set at all        OFF0  false when it reads 0        ON1  true when it reads 1
//   INT / LL / REAL  atoi / atoll / atof of the value (UNSET: absent, the planner decides)
//   INT3  "a,b,c" (missing fields stay 0)
#define SSN_PLAN_KNOBS(X)                                                                                                                          \
  X(PRESENT, debug_plan, "SSN_DEBUG_PLAN", false, "print the plan to stderr at ssn_create (and per-item times after a profile = 2 run)")          \
  X(INT, debug_deps, "SSN_DEBUG_DEPS", UNSET, "first of four pipelined rounds whose instances are printed with what they wait for")                \
  X(INT, ens_sweeps, "SSN_ENS_SWEEPS", UNSET, "256-thread sweeps per workgroup of an ensemble array (clamped to what the array has)")            \
  X(OFF0, small_ens, "SSN_SMALL_ENS", true, "a wave per ensemble for arrays of many small 1-D ensembles (RK_ENS_SMALL)")                          \
  X(INT3, block_variant, "SSN_BLOCK_VARIANT", Int3(), "tpb,npt,lds of the whole-block kernel variant to use")                                     \
  X(INT, block_split, "SSN_BLOCK_SPLIT", UNSET, "member workgroups per ensemble of the split whole-block kernel (1, 2, 4 or 8; others ignored)")  \
  X(INT, block_split_cus, "SSN_BLOCK_SPLIT_CUS", UNSET, "CU count the split is sized for (tests: pretend the GPU is smaller / larger)")           \
  X(ON1, block_sort, "SSN_BLOCK_SORT", false, "whole-block kernel: neurons in slot order (only pays with a SSN_BLOCK_SKIP build)")               \
  X(PRESENT, dft_no_inplace, "SSN_DFT_NO_INPLACE", false, "Bluestein transforms never in place")                                                  \
  X(INT, spmv_max_chunks, "SSN_SPMV_MAX_CHUNKS", 64, "most chunks of a segmented spike list per sparse decode (at least 1)")                     \
  X(LL, grid_min_mb, "SSN_GRID_MIN_MB", 64, "smallest clean-up table (MB) whose similarities come from the factored grid as an MFMA product")     \
  X(LL, grid_dot_min_mb, "SSN_GRID_DOT_MIN_MB", 16, "smallest clean-up table (MB) that goes through its factor tables as bodies of the round grid") \
  X(INT, grid_split, "SSN_GRID_SPLIT", UNSET, "K-split of the grid product (clamped to 1..8)")                                                    \
  X(INT, matvec_r1_max, "SSN_MATVEC_R1_MAX", 4096, "tallest matrix that runs four rows per workgroup in a round (taller: sixteen)")              \
  X(REAL, cost_pes, "SSN_COST_PES", 2.0, "balancer: fraction of its matrix a PES update is priced at")                                            \
  X(REAL, cost_voja, "SSN_COST_VOJA", 0.2, "balancer: fraction of its matrix a Voja update is priced at")                                         \
  X(REAL, lat_dft, "SSN_LAT_DFT", 9.0, "balancer: latency of a transform body (us)")                                                              \
  X(REAL, lat_solo, "SSN_LAT_SOLO", 3.0, "balancer: latency of a gate / argmax body (us)")                                                        \
  X(OFF0, pes_fold, "SSN_PES_FOLD", true, "fold the filter of a PES rule's activities into the rule's body")                                      \
  X(ON1, phased_pes_fold, "SSN_PHASED_PES_FOLD", false, "... also in neuron-sharded plans")                                                       \
  X(OFF0, fuse_neurons, "SSN_FUSE_NEURONS", true, "neuron update of a dense population in the epilogue of its encoder product")                   \
  X(INT, fuse_min_rows, "SSN_FUSE_MIN_ROWS", 4097, "smallest population that is fused so (tests lower it)")                                       \
  X(OFF0, solo_chains, "SSN_SOLO_CHAINS", true, "serial chains of single-workgroup operators (RK_SOLO)")                                          \
  X(OFF0, phased_solo, "SSN_PHASED_SOLO", true, "... in neuron-sharded plans")                                                                    \
  X(ON1, solo_dft, "SSN_SOLO_DFT", false, "transforms as members of serial chains (measured slower)")                                             \
  X(REAL, solo_cap_us, "SSN_SOLO_CAP_US", 16.0, "longest serial chain in estimated microseconds")                                                 \
  X(LL, solo_max_len, "SSN_SOLO_MAX_LEN", 2048, "longest glue operator (elements) a single workgroup takes")                                      \
  X(OFF0, round_interleave, "SSN_ROUND_INTERLEAVE", true, "interleaved dispatch of a round's big grids behind its latency-bound head")            \
  X(OFF0, head_prio, "SSN_HEAD_PRIO", true, "raised wave priority for the head blocks of a round")                                                \
  X(PRESENT, phase2_sequential, "SSN_PHASE2_SEQUENTIAL", false, "sharded: phase 1 of a timestep and phase 0 of the next as two sets of rounds")   \
  X(INT, cycle_steps, "SSN_CYCLE_STEPS", 16, "sharded: timesteps pipelined over the exchange (2..64; 0 or 1: off)")                               \
  X(PRESENT, no_batch_reorder, "SSN_NO_BATCH_REORDER", false, "time-batched stages keep the builder's operator order")                            \
  X(PRESENT, no_zero_skip, "SSN_NO_ZERO_SKIP", false, "time-batched products are multiplied out even when their whole input is zero")

struct PlanOptions {
  struct Int3 { int v[3] = {0, 0, 0}; };
  static constexpr int UNSET = INT_MIN;
  enum Kind { K_PRESENT, K_OFF0, K_ON1, K_INT, K_LL, K_REAL, K_INT3 };
  typedef bool T_PRESENT; typedef bool T_OFF0; typedef bool T_ON1; typedef int T_INT; typedef long long T_LL; typedef double T_REAL; typedef Int3 T_INT3;

  int flags = 0;                              // ssn_model_desc.flags (ssn_plan_flag bits)
#define X(kind, name, env, def, doc) T_##kind name = def;
  SSN_PLAN_KNOBS(X)
#undef X

  bool has(int bit) const { return (flags & bit) != 0; }

  static PlanOptions read(int flags) {
    PlanOptions o;
    o.flags = flags;
    struct Row { const char* env; Kind kind; void* field; };
#define X(kind, name, env, def, doc) {env, K_##kind, &o.name},
    const Row rows[] = {SSN_PLAN_KNOBS(X)};
#undef X
    for (const Row& k : rows) {
      const char* v = getenv(k.env);
      if (!v) continue;
      switch (k.kind) {
        case K_PRESENT: *(bool*)k.field = true; break;
        case K_OFF0: if (atoi(v) == 0) *(bool*)k.field = false; break;
        case K_ON1: if (atoi(v) == 1) *(bool*)k.field = true; break;
        case K_INT: *(int*)k.field = atoi(v); break;
        case K_LL: *(long long*)k.field = atoll(v); break;
        case K_REAL: *(double*)k.field = atof(v); break;
        case K_INT3: { Int3* t = (Int3*)k.field; sscanf(v, "%d,%d,%d", &t->v[0], &t->v[1], &t->v[2]); break; }
      }
    }
    return o;
  }
};

// A captured graph and its executable (Sim::capture_into fills it).
struct Graph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  Graph() = default;
  Graph(Graph&& o) noexcept : graph(o.graph), exec(o.exec) { o.graph = nullptr; o.exec = nullptr; }
  Graph(const Graph&) = delete;
  Graph& operator=(const Graph&) = delete;
  ~Graph() { reset(); }
  void reset() {
    if (exec) hipGraphExecDestroy(exec);
    if (graph) hipGraphDestroy(graph);
    exec = nullptr; graph = nullptr;
  }
};

// Device memory with one owner: a buffer that grows at run time (table rows and indices, probe storage), or a
// temporary.
struct DevBuf {
  void* p = nullptr;
  int64_t cap = 0;                            // bytes
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p) hipFree(p);
    p = nullptr; cap = 0;
  }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
  // a temporary of exactly `bytes` (not counted in ssn_counters.device_bytes)
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = (int64_t)bytes;
    return e;
  }
  // at least `need_bytes`: a buffer that is too small is freed and replaced (its contents are not kept)
  template <typename S>
  int grow(S& sim, int64_t need_bytes) {
    if (need_bytes <= cap) return SSN_OK;
    reset();
    CHK(sim.dmalloc(&p, need_bytes, false));
    cap = need_bytes;
    return SSN_OK;
  }
};

}  // namespace

struct ssn_sim {
  virtual ~ssn_sim() {}
  virtual int reset() = 0;
  virtual int set_table(int id, const double* rows, const void* rows_dev, int64_t n_rows, int64_t width,
                        const int32_t* idx, int64_t n_idx, int64_t first_step) = 0;
  virtual int stage_table(int id, const void* rows_t, int64_t n_rows, int64_t width, const int32_t* idx, int64_t n_idx, int64_t first_step) = 0;
  virtual int commit_tables() = 0;
  virtual int reserve_probes(int64_t n) = 0;
  virtual int run_steps(int64_t n, int profile) = 0;
  virtual int run_phase(int phase) = 0;
  virtual int64_t exchange_size() = 0;
  virtual int64_t cycle_len() = 0;
  virtual int exchange_copy(void* buf, bool pack) = 0;
  virtual int phase_async(int phase, void* buf, hipStream_t ext) = 0;
  virtual int phase_sync(hipStream_t ext) = 0;
  virtual int read_probe(int id, double* dst, void* dst_dev, int64_t first, int64_t count) = 0;
  virtual int64_t probe_count(int id) = 0;
  virtual int rw_signal(int64_t off, int64_t count, double* dst, const double* src) = 0;
  virtual int rw_buffer(int id, double* dst, const double* src, int64_t count) = 0;
  virtual int counters(ssn_counters* out) = 0;
  virtual int kernel_times(ssn_kernel_time* out, int capacity) = 0;
  virtual int64_t n_steps() = 0;
  virtual int buffer_view(int id, ssn::BufView* out) = 0;      // ssn_recall.hip: a matrix where it lies
};

namespace {

template <typename T>
struct Sim final : ssn_sim {
  using MOp = ssn::MicroOp<T>;
  static constexpr int VW = 16 / sizeof(T);

  struct TapSet;
  struct DriveSet;
  struct Item {
    int type = IT_PROGRAM;
    int op_begin = 0, op_count = 0;          // program: range in d_mops
    ssn::EnsArgs<T> ens;
    const TapSet* taps = nullptr;            // IT_ENS: the operator's neuron taps, if it has any (an entry of tap_sets)
    const DriveSet* drv = nullptr;           // IT_ENS: the operator's drive columns, if it has any (an entry of drive_sets)
    ssn::FinishArgs<T> fin;
    bool dominant = false;
    // matvec / pes / voja / neurons
    T* Wm = nullptr; const T* src = nullptr; T* dst = nullptr; const T* aux0 = nullptr; const T* aux1 = nullptr;
    const T* aux2 = nullptr; T* V = nullptr; T* R = nullptr;
    int rows = 0, cols = 0, ld = 0, set = 0, n = 0;
    T scalar = 0;
    ssn::NeuronParams<T> np;
    int* list = nullptr; int* count = nullptr;     // spike list (k_neurons_compact -> k_spmv_partial)
    int seg = 0;                                   // > 0: segmented spike list (k_neurons), segments per spmv chunk
    int seg_len = 256;                             // neurons per list segment (16: written by a fused product + neuron update)
    int level = -1;                                // scheduling round of the operator (builder): equal level = independent
    int phase = -1;                                // neuron-sharded models: 0 before the per-timestep exchange, 1 after (set by plan())
    T* lp_dst = nullptr; const T* lp_src = nullptr; T lp_a = 0, lp_b = 0;      // IT_PES: folded filter of the row factors (build_rounds)
    int batch = 1;                                 // this item and the next batch-1 items (same kind, independent) share one launch
    bool merged = false;                           // launched by the item that leads its batch
    ssn::DftArgs dft;
  };

  int device = 0;
  double dt = 0.001;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;          // downloads (see download())
  double* up_stage = nullptr;                 // device staging of upload() (float64 as it arrives from the host)
  int64_t up_cap = 0;
  void* dl_stage = nullptr;                   // pinned host staging of download()
  int64_t dl_cap = 0;
  std::mutex dl_mutex;
  int64_t n_sig = 0;
  T* sig = nullptr;
  std::vector<double> sig_init;
  std::vector<Buf> bufs;
  std::vector<Item> items;                   // one timestep of the core stage, unfused
  std::vector<void*> owned;                   // what ssn_create allocated (dmalloc): freed with the simulator
  // time-batched pre / post stages
  T* bsig = nullptr;                          // [block+1][n_sig]
  int block = 0;                              // timesteps per block (0: staging off)
  bool core_empty = false;                    // no per-timestep work at all
  const PlanOptions opt;                      // ssn_model_desc.flags and the environment knobs, as read at ssn_create
  bool fused_core = false;                    // core == one recurrent ensemble array: [k_ensarray, k_ens_finish]
  bool fused_defer = false;                   // ... with the finish deferred into the next step's prologue: [k_ensarray]
  ssn::FinishArgs<T> fin_begin, fin_flush;
  bool fused_block = false;                   // ... stepped a whole block per launch: [k_ens_block] (ssn_block.hpp)
  ssn::BlockArgs<T> blk;
  // neuron taps of the ensemble arrays (ssn_model_desc.taps, ABI 9): per tapped operator the table its kernels read -
  // [K][4] = first neuron, count (0: ensemble without a tap), destination signal, index among the operator's taps
  struct TapSet { std::vector<ssn_tap_desc> list; int* d_tab = nullptr; double amp = 0.0; };
  std::map<int, TapSet> tap_sets;             // operator index -> its taps
  // neuron-input drive columns of the ensemble arrays (ssn_drive_desc records, ABI 10): per driven operator its record, the
  // host copy of the column sources and the tables its kernel reads - [K][m][2] = signal offset (-1: unused), 1 if read from
  // the timestep's block row; d_tab reads everything from the signal vector, d_tab_rows (fused cores) the pre-stage signals
  // from the row
  struct DriveSet { ssn_drive_desc rec; std::vector<int32_t> src; int* d_tab = nullptr; int* d_tab_rows = nullptr; };
  std::map<int, DriveSet> drive_sets;         // operator index -> its drive columns
  std::set<int> sparse_w;                     // decoder buffers multiplied with a LIF spike vector
  std::set<int> learned_w;                    // matrices a learning rule (PES, Voja) updates
  std::vector<std::pair<int64_t, std::pair<int*, int*>>> spike_lists;   // spike signal offset -> (list, count)
  std::vector<int64_t> seg_spikes;                                       // spike signals whose list is segmented
  std::vector<std::pair<int64_t, float2*>> dft_tables;                  // dft_key(kind, sizes) -> table (twiddles, chirps, spectra, DFT matrices)
  std::vector<ssn::BatchOp<T>> pre_ops, post_ops;
  std::vector<ssn::stage::Launch> pre_launches, post_launches;      // the launches over them (optimise_batch)
  int batch_skipped = 0;                     // products of the batched stages whose whole input was zero over a block (run_batch)
  std::vector<ssn_range> pre_to_core, core_to_post;
  std::vector<unsigned char> batched_mask;    // signals owned by a batched stage (for ssn_read_signal)
  std::vector<MOp> mops;                     // [head][middle programs...][tail][head copy]
  MOp* d_mops = nullptr;
  std::vector<ssn::ProgDesc> prog_descs;     // one per program (+ a copy of the head behind the tail)
  ssn::ProgDesc* d_progs = nullptr;
  std::vector<std::pair<const void*, std::pair<const int32_t*, int64_t>>> host_idx;   // device idx ptr -> host copy
  int head_begin = 0, head_count = 0, tail_begin = 0, tail_count = 0;
  bool can_fuse = false;
  // generic plan: which earlier items of the timestep each item must wait for (data hazards on signal ranges,
  // buffers and scratch memory) - lets the step graph fork independent branches over several streams
  struct Rng { const void* space; int64_t lo, hi; bool w; };
  std::vector<std::vector<int>> item_deps;
  std::vector<MOp> vecops_host;               // operators of the grid-wide first level (IT_VECOPS), host copy
  std::map<const void*, std::vector<ssn::LinTerm<T>>> lin_terms;   // device term list of a M_LINCOMB operator -> host copy
  // round plan (k_round, ssn_round.hpp): every launch of a timestep, in order
  struct RoundLaunch { ssn::RoundArgs<T> args; int n_blocks = 0; size_t lds = 0; int round = 0; };
  struct Launch { int rl = -1; int item = -1; int phase = 0; };
  bool round_mode = false;
  std::vector<RoundLaunch> round_launches;
  std::vector<Launch> launch_list;            // one timestep (item plans: one entry per unmerged item)
  std::vector<Launch> graph_list;             // steps_per_graph timesteps, software-pipelined (empty: replay launch_list)
  // neuron-sharded models, pipelined (round 4): cycle_steps timesteps as cycle_steps + 1 launch segments; the caller's exchange of
  // timestep k sits between segments k and k + 1 (ssn_run_phase / ssn_phase_async with phase 3 = "the next segment")
  std::vector<std::vector<Launch>> cycle_segs;
  int cycle_steps = 0, next_seg = 0;
  int n_fused_populations = 0, n_serial_chains = 0;      // (counters of the round plan)
  std::vector<Graph> cycle_graph;             // (stream-ordered stepping: one per segment)
  std::vector<Launch> phase2_list;            // neuron-sharded models: the updates of timestep s and timestep s + 1 up to its exchange,
                                              // planned as ONE set of rounds (empty: the two halves one after the other)
  int graph_rounds = 0;

  ssn::StepCtx* d_ctx = nullptr;
  std::vector<ssn::TableSlot> tables;
  // host copy of every table's row index per step: a time-batched product whose whole input is a table that is zero for the
  // whole block (the init-SSP input of the path integrator after its first 50 ms, reference run_pathint.py:136) is not
  // multiplied out - its result rows are zero-filled instead
  std::vector<std::vector<int32_t>> table_idx_host;
  ssn::TableSlot* d_tables = nullptr;
  std::vector<DevBuf> table_rows, table_idx;
  // staged tables (ssn_stage_table / ssn_commit_tables): the NEXT chunk's inputs arrive in a second set of buffers by DMA on the
  // copy stream while the compute stream still reads the current ones; commit swaps the sets between two runs
  struct Staged { DevBuf rows, idx; bool valid = false;
                  int64_t n_rows = 0, width = 0, n_idx = 0, first_step = 0; std::vector<int32_t> idx_host; };
  std::vector<Staged> staged;
  std::mutex stage_mutex;
  std::vector<ssn_probe_desc> probes;
  std::vector<ssn::ProbeSlot> pslots;
  ssn::ProbeSlot* d_pslots = nullptr;
  std::vector<DevBuf> probe_store;            // pslots[p].data
  int64_t reserve_first = 0, reserve_n = 0;
  int steps_per_graph = 0;
  Graph step_graph;                           // steps_per_graph timesteps
  int64_t steps_done = 0;
  int64_t device_bytes = 0;
  // timing
  hipEvent_t ev_run0 = nullptr, ev_run1 = nullptr;
  std::vector<hipEvent_t> ev_pool;
  int64_t dom_launches = 0;
  double dom_ms = 0.0, last_run_ms = 0.0;
  double dom_bytes = 0.0;
  int64_t dom_units = 0;
  int launches_per_step = 0;
  // neuron-sharded model: the timestep's items in two halves around the caller's all-reduce
  std::vector<ssn_range> exchange;
  bool phased = false;
  int next_phase = 0;
  Graph phase_graph[3];                       // [2]: phase 1 of a timestep followed by phase 0 of the next
  // stream-ordered stepping (ssn_phase_async): the same halves with the exchange copies inside the graph, for one exchange
  // buffer of the caller; launched on the caller's stream, no host synchronisation per timestep
  Graph async_graph[3];
  void* async_buf = nullptr;
  bool async_captured = false, async_active = false;
  hipStream_t async_stream = nullptr;         // the caller's stream a stream-ordered run is in flight on (while async_active)
  static constexpr int N_ITEM_TYPES = 18;
  double type_ms[N_ITEM_TYPES] = {};             // profile = 2: device time per plan-item type
  int64_t type_launches[N_ITEM_TYPES] = {};
  std::vector<double> item_ms;                   // ... and per plan item (printed under SSN_DEBUG_PLAN)
  std::vector<int64_t> item_n;

  explicit Sim(const ssn_model_desc* m) : opt(PlanOptions::read(m->flags)) {}

  ~Sim() override {
    hipSetDevice(device);
    if (async_active && async_stream) hipStreamSynchronize(async_stream);
    if (stream) hipStreamSynchronize(stream);
    // graphs, then device memory, then events; the copy stream and the staging it fills; the compute stream last
    step_graph.reset();
    for (int h = 0; h < 3; ++h) { phase_graph[h].reset(); async_graph[h].reset(); }
    cycle_graph.clear();
    table_rows.clear(); table_idx.clear(); staged.clear(); probe_store.clear();
    for (void* p : owned) hipFree(p);
    for (auto e : ev_pool) hipEventDestroy(e);
    if (ev_run0) hipEventDestroy(ev_run0);
    if (ev_run1) hipEventDestroy(ev_run1);
    if (copy_stream) { hipStreamSynchronize(copy_stream); hipStreamDestroy(copy_stream); }
    if (dl_stage) hipHostFree(dl_stage);
    if (up_stage) hipFree(up_stage);
    if (stream) hipStreamDestroy(stream);
  }

  // Device memory, counted in ssn_counters.device_bytes.  Owned: the simulator frees it when it is destroyed - every
  // allocation of ssn_create, the only writer of `owned`.  Not owned (DevBuf::grow): the caller frees it.
  template <typename P>
  int dmalloc(P** p, int64_t bytes, bool own = true) {
    if (bytes <= 0) bytes = 16;
    HIPCHK(hipMalloc((void**)p, (size_t)bytes));
    device_bytes += bytes;
    if (own) owned.push_back((void*)*p);
    return SSN_OK;
  }
  // A host table on the device: owned memory for n elements of P, filled from `src` / with zeros (n = 0: dmalloc's 16 bytes).
  template <typename P>
  int dupload(P** p, const P* src, int64_t n) {
    CHK(dmalloc(p, n * (int64_t)sizeof(P)));
    if (n > 0) HIPCHK(hipMemcpy(*p, src, (size_t)n * sizeof(P), hipMemcpyHostToDevice));
    return SSN_OK;
  }
  template <typename P>
  int dupload(P** p, const std::vector<P>& v) { return dupload(p, v.data(), (int64_t)v.size()); }
  template <typename P>
  int dzeros(P** p, int64_t n) {
    CHK(dmalloc(p, n * (int64_t)sizeof(P)));
    if (n > 0) HIPCHK(hipMemset(*p, 0, (size_t)n * sizeof(P)));
    return SSN_OK;
  }

  // host double[rows*cols] -> device T[rows*ld]
  int upload(const double* src, T* dst, int64_t rows, int64_t cols, int64_t ld) {
    const int64_t n = rows * cols;
    if (n == 0) return SSN_OK;
    // float64 staging on the device: uploads of up to 64 MB share one buffer that stays (the tables of a chunked run are
    // replaced at every chunk boundary - a hipMalloc / hipFree pair per table there cost more than the copy); larger ones
    // (weight matrices at build time, config 5's 14 GB clean-up table) take and release their own
    constexpr int64_t KEEP = (int64_t)8 << 20;                 // elements
    double* stage = nullptr;
    DevBuf own;
    if (n <= KEEP) {
      if (n > up_cap) {
        if (up_stage) { hipFree(up_stage); up_stage = nullptr; up_cap = 0; }
        const int64_t want = std::min<int64_t>(KEEP, std::max<int64_t>(2 * n, 1 << 16));
        HIPCHK(hipMalloc((void**)&up_stage, (size_t)want * sizeof(double)));
        up_cap = want;
      }
      stage = up_stage;
    } else {
      HIPCHK(own.alloc((size_t)n * sizeof(double)));
      stage = (double*)own.p;
    }
    hipError_t e = hipMemcpyAsync(stage, src, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = ssn::launch_convert_in<T>(stream, stage, dst, rows, cols, ld);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    HIPCHK(e);
    return SSN_OK;
  }

  // Device -> host as float64.  The values travel in the simulator's own type into a pinned host buffer (a DMA copy on a
  // stream of its own: no kernel, so it does not queue behind a compute kernel that owns every CU, and no pageable
  // staging) and are widened on the host by a few threads.  A caller thread may therefore fetch the probe samples of the
  // timesteps that are done while another thread's ssn_run_steps steps the next ones (simulator.py does, chunk by
  // chunk).  Everything read here was completed by a call that synchronised the compute stream before it returned.
  int download(const T* src, double* dst, int64_t rows, int64_t cols, int64_t ld) {
    const int64_t n = rows * cols;
    if (n == 0) return SSN_OK;
    std::lock_guard<std::mutex> lock(dl_mutex);
    if (!copy_stream) HIPCHK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    if (n > dl_cap) {
      if (dl_stage) { HIPCHK(hipStreamSynchronize(copy_stream)); hipHostFree(dl_stage); dl_stage = nullptr; }
      const int64_t want = std::max<int64_t>(n, 1 << 20);
      HIPCHK(hipHostMalloc((void**)&dl_stage, (size_t)want * sizeof(T), hipHostMallocDefault));
      dl_cap = want;
    }
    T* h = (T*)dl_stage;
    if (ld == cols) HIPCHK(hipMemcpyAsync(h, src, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, copy_stream));
    else HIPCHK(hipMemcpy2DAsync(h, (size_t)cols * sizeof(T), src, (size_t)ld * sizeof(T), (size_t)cols * sizeof(T), (size_t)rows, hipMemcpyDeviceToHost, copy_stream));
    HIPCHK(hipStreamSynchronize(copy_stream));
    auto widen = [h, dst](int64_t lo, int64_t hi) { for (int64_t i = lo; i < hi; ++i) dst[i] = (double)h[i]; };
    const int nt = n >= (1 << 21) ? 4 : 1;
    if (nt == 1) { widen(0, n); return SSN_OK; }
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(widen, n * t / nt, n * (t + 1) / nt);
    widen(0, n / nt);
    for (auto& th : pool) th.join();
    return SSN_OK;
  }

  bool ens_fast(const ssn_op_desc& o) const {
    // spiking LIF with min_voltage == 0: packed state word + (dout >= 3) spike-sparse neuron-major decoders
    return !opt.has(SSN_PLAN_NO_LIF_FAST) && o.i[11] == SSN_LIF && o.f[2] == 0.0;
  }

  bool ens_sparse(const ssn_op_desc& o) const { return ens_fast(o) && !opt.has(SSN_PLAN_DENSE_DECODERS) && o.i[4] >= 3; }

  // host [rows][cols] double -> device layout of buffer b
  int upload_buf(Buf& b, const double* src) {
    std::vector<double> ordered;
    if (b.perm) {                      // the device's neuron order (columns permuted within every ensemble's rows)
      ordered.resize((size_t)(b.rows * b.cols));
      const int32_t* pm = b.perm->data();
      for (int64_t r = 0; r < b.rows; ++r) {
        const int32_t* pk = pm + (r / b.perm_rows) * b.cols;
        const double* in = src + r * b.cols;
        double* out = ordered.data() + r * b.cols;
        for (int64_t c = 0; c < b.cols; ++c) out[c] = in[pk[c]];
      }
      src = ordered.data();
    }
    if (b.transposed) {
      DevBuf own;
      HIPCHK(own.alloc((size_t)(b.rows * b.ld) * sizeof(T)));
      T* tmp = (T*)own.p;
      int rc = upload(src, tmp, b.rows, b.cols, b.ld);
      hipError_t e = hipSuccess;
      if (rc == SSN_OK) e = hipMemsetAsync(b.d, 0, (size_t)(b.cols * b.ldt) * sizeof(T), stream);
      if (rc == SSN_OK && e == hipSuccess) e = ssn::launch_transpose<T>(stream, tmp, (T*)b.d, (int)b.rows, (int)b.cols, (int)b.ld, (int)b.ldt);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      CHK(rc);
      HIPCHK(e);
      return SSN_OK;
    }
    if (!b.dec_DP) return upload(src, (T*)b.d, b.rows, b.cols, b.ld);
    DevBuf own;
    HIPCHK(own.alloc((size_t)(b.rows * b.ld) * sizeof(T)));
    T* tmp = (T*)own.p;
    int rc = upload(src, tmp, b.rows, b.cols, b.ld);
    hipError_t e = hipSuccess;
    if (rc == SSN_OK) e = ssn::launch_dec_pack<T>(stream, tmp, (T*)b.d, b.dec_K, b.dec_dout, b.dec_n, (int)b.ld, b.dec_DP, 0);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    CHK(rc);
    HIPCHK(e);
    return SSN_OK;
  }

  int download_buf(Buf& b, double* dst) {
    if (b.perm) {                      // back to the caller's neuron order
      std::shared_ptr<std::vector<int32_t>> pm = b.perm;
      b.perm.reset();
      std::vector<double> dev((size_t)(b.rows * b.cols));
      const int rc = download_buf(b, dev.data());
      b.perm = pm;
      CHK(rc);
      for (int64_t r = 0; r < b.rows; ++r) {
        const int32_t* pk = pm->data() + (r / b.perm_rows) * b.cols;
        const double* in = dev.data() + r * b.cols;
        double* out = dst + r * b.cols;
        for (int64_t c = 0; c < b.cols; ++c) out[pk[c]] = in[c];
      }
      return SSN_OK;
    }
    if (b.transposed) {
      DevBuf own;
      HIPCHK(own.alloc((size_t)(b.rows * b.ld) * sizeof(T)));
      T* tmp = (T*)own.p;
      hipError_t e = ssn::launch_transpose<T>(stream, (const T*)b.d, tmp, (int)b.cols, (int)b.rows, (int)b.ldt, (int)b.ld);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);          // (download() copies on its own stream)
      int rc = e == hipSuccess ? download(tmp, dst, b.rows, b.cols, b.ld) : SSN_OK;
      HIPCHK(e);
      return rc;
    }
    if (!b.dec_DP && !b.packed) return download((const T*)b.d, dst, b.rows, b.cols, b.ld);
    DevBuf own;
    HIPCHK(own.alloc((size_t)(b.rows * b.ld) * sizeof(T)));
    T* tmp = (T*)own.p;
    hipError_t e = hipSuccess;
    if (b.dec_DP) {
      e = hipMemsetAsync(tmp, 0, (size_t)(b.rows * b.ld) * sizeof(T), stream);
      if (e == hipSuccess) e = ssn::launch_dec_pack<T>(stream, (const T*)b.d, tmp, b.dec_K, b.dec_dout, b.dec_n, (int)b.ld, b.dec_DP, 1);
    } else {
      const T* words = (const T*)(b.packed == 2 ? bufs[b.partner].d : b.d);
      // (the f32 whole-block kernel keeps -(R - dt) in the state word of a refractory neuron, every other kernel -R)
      e = ssn::launch_state_unpack<T>(stream, words, tmp, b.rows * b.ld, b.packed == 2, (fused_block && sizeof(T) == 4) ? (T)dt : T(0));
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);            // (download() copies on its own stream)
    int rc = e == hipSuccess ? download(tmp, dst, b.rows, b.cols, b.ld) : SSN_OK;
    HIPCHK(e);
    return rc;
  }

  int shape(int id, int64_t rows, int64_t cols, bool pad, bool keep) {
    if (id < 0 || id >= (int)bufs.size()) return fail(SSN_EINVAL, "buffer id %d out of range", id);
    Buf& b = bufs[id];
    if (sparse_w.count(id)) { b.transposed = true; b.ldt = (rows + VW - 1) / VW * VW; pad = true; }
    if (b.kind != SSN_BUF_REAL) return fail(SSN_EINVAL, "buffer %d is not a real buffer", id);
    if (rows * cols != b.count) return fail(SSN_EINVAL, "buffer %d has %lld elements, operator expects %lld x %lld",
                                            id, (long long)b.count, (long long)rows, (long long)cols);
    const int64_t ld = pad ? (cols + VW - 1) / VW * VW : cols;
    if (b.shaped && (b.rows != rows || b.cols != cols || b.ld != ld))
      return fail(SSN_EINVAL, "buffer %d is used with two different layouts", id);
    b.rows = rows; b.cols = cols; b.ld = ld; b.shaped = true;
    b.keep = b.keep || keep;
    return SSN_OK;
  }

  static bool is_micro(const ssn_op_desc& o) {
    switch (o.kind) {
      case SSN_OP_FILL: case SSN_OP_TABLE: case SSN_OP_AXPY: case SSN_OP_LOWPASS: case SSN_OP_GATE: case SSN_OP_LINCOMB: return true;
      case SSN_OP_MATVEC: return o.i[3] <= 16 && o.i[2] <= 8192;
      default: return false;
    }
  }

  int check_range(int64_t off, int64_t len, const char* what) {
    if (off < 0 || len < 0 || off + len > n_sig) return fail(SSN_EINVAL, "%s range [%lld,+%lld) outside the %lld signals",
                                                             what, (long long)off, (long long)len, (long long)n_sig);
    return SSN_OK;
  }

  // Taps (ABI 9): every range inside its array and inside the signal vector, one tap per ensemble, tap signals disjoint
  // from each other and from every decoded row of an array.
  int read_taps(const ssn_model_desc* m) {
    for (int i = 0; i < m->n_buffers; ++i)
      if (m->buffers[i].kind == SSN_BUF_TAPS && (m->n_taps <= 0 || i != m->n_buffers - 1))
        return fail(SSN_EINVAL, "buffer %d: tap records belong in the last buffer of a model with n_taps > 0", i);
    if (m->n_taps < 0) return fail(SSN_EINVAL, "n_taps = %d", m->n_taps);
    if (m->n_taps == 0) return SSN_OK;
    const ssn_buffer_desc& tb = m->buffers[m->n_buffers > 0 ? m->n_buffers - 1 : 0];
    if (m->n_buffers < 1 || tb.kind != SSN_BUF_TAPS || tb.count != m->n_taps || !tb.data)
      return fail(SSN_EINVAL, "n_taps = %d: the last buffer must hold that many ssn_tap_desc records (SSN_BUF_TAPS)", m->n_taps);
    const ssn_tap_desc* const tap_list = (const ssn_tap_desc*)tb.data;
    if (opt.has(SSN_PLAN_SPLIT_BLOCK))
      return fail(SSN_EUNSUPPORTED, "SSN_PLAN_SPLIT_BLOCK does not go with neuron taps (the split whole-block kernel has no tapped form)");
    std::vector<unsigned char> mark((size_t)n_sig, 0);
    for (int i = 0; i < m->n_taps; ++i) {
      const ssn_tap_desc& t = tap_list[i];
      if (t.op < 0 || t.op >= m->n_ops || m->ops[t.op].kind != SSN_OP_ENSARRAY || m->ops[t.op].stage != 1)
        return fail(SSN_EINVAL, "tap %d: operator %d is not an ensemble array of the per-timestep core", i, t.op);
      const ssn_op_desc& o = m->ops[t.op];
      if (t.k < 0 || t.k >= o.i[1]) return fail(SSN_EINVAL, "tap %d: ensemble %d outside the array's %lld", i, t.k, (long long)o.i[1]);
      if (t.first < 0 || t.count < 1 || t.first + t.count > o.i[2])
        return fail(SSN_EINVAL, "tap %d: neurons [%lld,+%lld) outside the ensemble's %lld", i, (long long)t.first, (long long)t.count, (long long)o.i[2]);
      CHK(check_range(t.dst, t.count, "tap"));
      TapSet& ts = tap_sets[t.op];
      for (const ssn_tap_desc& q : ts.list)
        if (q.k == t.k) return fail(SSN_EINVAL, "tap %d: ensemble %d of operator %d already has a tap", i, t.k, t.op);
      if (!ts.list.empty() && ts.amp != t.amp) return fail(SSN_EINVAL, "tap %d: the taps of one array share one amplitude", i);
      ts.amp = t.amp;
      ts.list.push_back(t);
      for (int64_t e = t.dst; e < t.dst + t.count; ++e) {
        if (mark[(size_t)e]) return fail(SSN_EINVAL, "tap %d: its signal range overlaps another tap's", i);
        mark[(size_t)e] = 1;
      }
    }
    for (int i = 0; i < m->n_ops; ++i) {
      const ssn_op_desc& o = m->ops[i];
      if (o.kind != SSN_OP_ENSARRAY) continue;
      const int32_t* di = (const int32_t*)m->buffers[o.i[8]].data;
      for (int64_t j = 0; j < o.i[1] * o.i[4]; ++j)
        if (mark[(size_t)di[j]]) return fail(SSN_EINVAL, "a tap's signal range overlaps a decoded row of operator %d", i);
    }
    for (auto& kv : tap_sets) {
      const int64_t K = m->ops[kv.first].i[1];
      std::vector<int> tab((size_t)K * 4, 0);
      for (size_t q = 0; q < kv.second.list.size(); ++q) {
        const ssn_tap_desc& t = kv.second.list[q];
        int* row = tab.data() + (size_t)t.k * 4;
        row[0] = (int)t.first; row[1] = (int)t.count; row[2] = (int)t.dst; row[3] = (int)q;
      }
      CHK(dupload(&kv.second.d_tab, tab));
    }
    return SSN_OK;
  }
  // Drive columns (ABI 10): the records are found by the buffer's kind; every record names a core ensemble array (one record per
  // operator), 1 <= m <= 4, a real buffer of K * m * n weights and an int32 buffer of K * m sources inside the signal vector or -1.
  int read_drives(const ssn_model_desc* m) {
    int at = -1;
    for (int i = 0; i < m->n_buffers; ++i)
      if (m->buffers[i].kind == SSN_BUF_DRIVES) {
        if (at >= 0) return fail(SSN_EINVAL, "buffers %d and %d: at most one buffer of drive records (SSN_BUF_DRIVES)", at, i);
        at = i;
      }
    if (at < 0) return SSN_OK;
    const ssn_buffer_desc& db = m->buffers[at];
    if (db.count < 1 || !db.data) return fail(SSN_EINVAL, "buffer %d: a drive buffer holds at least one ssn_drive_desc record", at);
    if (opt.has(SSN_PLAN_SPLIT_BLOCK))
      return fail(SSN_EUNSUPPORTED, "SSN_PLAN_SPLIT_BLOCK does not go with neuron-input drive columns (the whole-block kernel has no driven form)");
    const ssn_drive_desc* const list = (const ssn_drive_desc*)db.data;
    for (int64_t i = 0; i < db.count; ++i) {
      const ssn_drive_desc& d = list[i];
      if (d.op < 0 || d.op >= m->n_ops || m->ops[d.op].kind != SSN_OP_ENSARRAY || m->ops[d.op].stage != 1)
        return fail(SSN_EINVAL, "drive %lld: operator %d is not an ensemble array of the per-timestep core", (long long)i, d.op);
      if (drive_sets.count(d.op)) return fail(SSN_EINVAL, "drive %lld: operator %d already has a drive record", (long long)i, d.op);
      if (d.m < 1 || d.m > ssn::ENS_DRIVE_MAX) return fail(SSN_EINVAL, "drive %lld: m = %d columns (1 .. %d)", (long long)i, d.m, ssn::ENS_DRIVE_MAX);
      const ssn_op_desc& o = m->ops[d.op];
      const int64_t K = o.i[1], n = o.i[2];
      if (d.w_buf < 0 || d.w_buf >= m->n_buffers || m->buffers[d.w_buf].kind != SSN_BUF_REAL || m->buffers[d.w_buf].count != K * d.m * n)
        return fail(SSN_EINVAL, "drive %lld: w_buf must be a real buffer of K * m * n = %lld weights", (long long)i, (long long)(K * d.m * n));
      if (d.src_buf < 0 || d.src_buf >= m->n_buffers || m->buffers[d.src_buf].kind != SSN_BUF_I32 || m->buffers[d.src_buf].count != K * d.m)
        return fail(SSN_EINVAL, "drive %lld: src_buf must be an int32 buffer of K * m = %lld sources", (long long)i, (long long)(K * d.m));
      const int32_t* src = (const int32_t*)m->buffers[d.src_buf].data;
      for (int64_t j = 0; j < K * d.m; ++j)
        if (src[j] < -1 || src[j] >= n_sig) return fail(SSN_EINVAL, "drive %lld: source %lld = %d outside the %lld signals (-1: unused)", (long long)i, (long long)j, src[j], (long long)n_sig);
      CHK(shape(d.w_buf, K * d.m, n, true, false));          // rows padded like enc's
      if (bufs[d.w_buf].ld != bufs[o.i[5]].ld) return fail(SSN_EINVAL, "drive %lld: weight rows and encoder rows are padded differently", (long long)i);
      DriveSet& ds = drive_sets[d.op];
      ds.rec = d;
      ds.src.assign(src, src + K * d.m);
    }
    return SSN_OK;
  }
  // the device tables of the drive columns (once the boundary ranges are known: before plan())
  int drive_tables() {
    for (auto& kv : drive_sets) {
      DriveSet& ds = kv.second;
      std::vector<int> tab(ds.src.size() * 2, 0), rows(ds.src.size() * 2, 0);
      for (size_t j = 0; j < ds.src.size(); ++j) {
        tab[2 * j] = rows[2 * j] = ds.src[j];
        for (auto& r : pre_to_core) if (ds.src[j] >= r.lo && ds.src[j] < r.hi) rows[2 * j + 1] = 1;
      }
      CHK(dupload(&ds.d_tab, tab));
      CHK(dupload(&ds.d_tab_rows, rows));
    }
    return SSN_OK;
  }
  // the drive columns / the taps of operator `op` of the model (nullptr: it has none)
  const DriveSet* drives_of(int op) const {
    auto it = drive_sets.find(op);
    return it == drive_sets.end() ? nullptr : &it->second;
  }
  const TapSet* taps_of(int op) const {
    auto it = tap_sets.find(op);
    return it == tap_sets.end() ? nullptr : &it->second;
  }

  int create(const ssn_model_desc* m) {
    device = m->device;
    dt = m->dt;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&ev_run0));
    HIPCHK(hipEventCreate(&ev_run1));
    n_sig = m->n_signals;
    if (n_sig >= (1LL << 31)) return fail(SSN_EINVAL, "%lld signals: the vector operators index with 32 bits", (long long)n_sig);
    sig_init.assign(m->signal_init, m->signal_init + n_sig);
    CHK(dmalloc(&sig, (n_sig + 8) * (int64_t)sizeof(T)));
    bufs.resize(m->n_buffers);
    for (int i = 0; i < m->n_buffers; ++i) {
      bufs[i].count = m->buffers[i].count;
      bufs[i].kind = m->buffers[i].kind;
      bufs[i].cols = bufs[i].ld = bufs[i].count;
      if (!m->buffers[i].data && bufs[i].count) return fail(SSN_EINVAL, "buffer %d has no data", i);
    }
    for (int i = 0; i < m->n_ops; ++i)
      if (m->ops[i].kind == SSN_OP_PES || m->ops[i].kind == SSN_OP_VOJA) learned_w.insert((int)m->ops[i].i[0]);
    // decoders applied to the spike vector of a dense LIF ensemble are kept neuron-major and multiplied sparsely
    if (!opt.has(SSN_PLAN_NO_SPMV))
      for (int i = 0; i < m->n_ops; ++i) {
        const ssn_op_desc& o = m->ops[i];
        if (o.kind != SSN_OP_MATVEC || o.stage != 1 || is_micro(o) || o.i[3] < 128) continue;
        if (o.i[3] > 15000 && opt.has(SSN_PLAN_SPMV_OWN_LIST)) continue;      // (a spike list rebuilt inside k_spmv_partial lives in LDS)
        for (int j = 0; j < m->n_ops; ++j) {
          const ssn_op_desc& q = m->ops[j];
          if (q.kind == SSN_OP_NEURONS && q.i[5] == SSN_LIF && q.i[1] == o.i[1] && q.i[2] == o.i[3]) sparse_w.insert((int)o.i[4]);
        }
      }
    for (int i = 0; i < m->n_ops; ++i) {          // a buffer also used as a dense operand elsewhere stays dense
      const ssn_op_desc& o = m->ops[i];
      if (o.kind == SSN_OP_MATVEC && sparse_w.count((int)o.i[4])) {
        bool ok = false;
        for (int j = 0; j < m->n_ops; ++j) {
          const ssn_op_desc& q = m->ops[j];
          if (q.kind == SSN_OP_NEURONS && q.i[5] == SSN_LIF && q.i[1] == o.i[1] && q.i[2] == o.i[3] && o.stage == 1 && !is_micro(o)) ok = true;
        }
        if (!ok) sparse_w.erase((int)o.i[4]);
      }
      if ((o.kind == SSN_OP_VOJA || o.kind == SSN_OP_CLEANUP) && sparse_w.count((int)o.i[o.kind == SSN_OP_VOJA ? 0 : 4])) sparse_w.erase((int)o.i[o.kind == SSN_OP_VOJA ? 0 : 4]);
    }
    // pass 1: buffer layouts
    for (int i = 0; i < m->n_ops; ++i) {
      const ssn_op_desc& o = m->ops[i];
      switch (o.kind) {
        case SSN_OP_ENSARRAY: {
          const int64_t K = o.i[1], n = o.i[2], din = o.i[3], dout = o.i[4];
          if (din < 1 || din > 4 || dout < 1 || dout > 8)
            return fail(SSN_EUNSUPPORTED, "ensemble array with din=%lld dout=%lld (kernels cover din<=4, dout<=8)",
                        (long long)din, (long long)dout);
          CHK(shape((int)o.i[5], K * din, n, true, false));
          CHK(shape((int)o.i[6], K, n, true, false));
          CHK(shape((int)o.i[7], K * dout, n, true, false));
          CHK(shape((int)o.i[9], K, n, true, true));
          CHK(shape((int)o.i[10], K, n, true, true));
          if (ens_fast(o)) {
            Buf& vb = bufs[o.i[9]]; Buf& rb = bufs[o.i[10]]; Buf& db = bufs[o.i[7]];
            if (vb.packed == 2 || rb.packed == 1 || o.i[9] == o.i[10]) return fail(SSN_EINVAL, "ensemble array state buffers shared inconsistently");
            vb.packed = 1; rb.packed = 2; rb.partner = (int)o.i[9];
            if (ens_sparse(o)) { db.dec_K = (int)K; db.dec_dout = (int)dout; db.dec_n = (int)n; db.dec_DP = dout <= 4 ? 4 : 8; }
          }
          if (o.i[8] < 0 || o.i[8] >= m->n_buffers || bufs[o.i[8]].kind != SSN_BUF_I32 || bufs[o.i[8]].count != K * dout)
            return fail(SSN_EINVAL, "ensemble array dst_idx buffer must be int32 [K*dout]");
          const int32_t* di = (const int32_t*)m->buffers[o.i[8]].data;
          for (int64_t j = 0; j < K * dout; ++j)
            if (di[j] < 0 || di[j] >= n_sig) return fail(SSN_EINVAL, "ensemble array destination index out of range");
          CHK(check_range(o.i[0], K * din, "ensarray x"));
          break;
        }
        case SSN_OP_MATVEC:
          // (a matrix that a learning rule updates keeps that rule's padded rows also when its product is small enough to run as a
          //  glue micro-operator - those read it with the buffer's leading dimension: found by the random-network tests, round 4)
          CHK(shape((int)o.i[4], o.i[2], o.i[3], !is_micro(o) || learned_w.count((int)o.i[4]) != 0, false));
          CHK(check_range(o.i[0], o.i[2], "matvec dst"));
          CHK(check_range(o.i[1], o.i[3], "matvec src"));
          break;
        case SSN_OP_NEURONS:
          CHK(shape((int)o.i[3], 1, o.i[2], false, true));
          CHK(shape((int)o.i[4], 1, o.i[2], false, true));
          CHK(check_range(o.i[0], o.i[2], "neurons J"));
          CHK(check_range(o.i[1], o.i[2], "neurons out"));
          break;
        case SSN_OP_PES:
          CHK(shape((int)o.i[0], o.i[1], o.i[2], true, true));
          CHK(check_range(o.i[3], o.i[1], "pes err"));
          CHK(check_range(o.i[4], o.i[2], "pes act"));
          break;
        case SSN_OP_VOJA:
          CHK(shape((int)o.i[0], o.i[1], o.i[2], true, true));
          CHK(shape((int)o.i[6], 1, o.i[1], false, false));
          CHK(check_range(o.i[3], o.i[1], "voja spikes"));
          CHK(check_range(o.i[4], o.i[2], "voja key"));
          CHK(check_range(o.i[5], 1, "voja learn"));
          break;
        case SSN_OP_CLEANUP:
          CHK(shape((int)o.i[4], o.i[2], o.i[3], true, false));
          if (o.i[5] > 0) {       // factor tables of the sample grid: dft (2K x d), lhs (n_a x 2K), rhs (N x 2K), n_a * N = rows
            if (o.i[8] <= 0 || o.i[9] <= 0 || o.i[10] <= 0 || (o.i[10] & 1) || o.i[8] * o.i[9] != o.i[2])
              return fail(SSN_EINVAL, "cleanup grid factors %lld x %lld (2K = %lld) do not match the %lld-row table",
                          (long long)o.i[8], (long long)o.i[9], (long long)o.i[10], (long long)o.i[2]);
            CHK(shape((int)o.i[5] - 1, o.i[10], o.i[3], true, false));
            CHK(shape((int)o.i[6] - 1, o.i[8], o.i[10], true, false));
            CHK(shape((int)o.i[7] - 1, o.i[9], o.i[10], true, false));
          }
          CHK(check_range(o.i[0], o.i[3], "cleanup dst"));
          CHK(check_range(o.i[1], o.i[3], "cleanup src"));
          break;
        case SSN_OP_FILL: CHK(check_range(o.i[0], o.i[1], "fill")); break;
        case SSN_OP_TABLE:
          CHK(check_range(o.i[0], o.i[1], "table"));
          if (o.i[2] < 0 || o.i[2] >= m->n_tables) return fail(SSN_EINVAL, "table id out of range");
          break;
        case SSN_OP_AXPY: CHK(check_range(o.i[0], o.i[2], "axpy dst")); CHK(check_range(o.i[1], o.i[2], "axpy src")); break;
        case SSN_OP_LOWPASS: CHK(check_range(o.i[0], o.i[2], "lowpass dst")); CHK(check_range(o.i[1], o.i[2], "lowpass src")); break;
        case SSN_OP_GATE: CHK(check_range(o.i[0], o.i[2], "gate dst")); CHK(check_range(o.i[1], 2 * o.i[2] + 1, "gate src")); break;
        case SSN_OP_LINCOMB: {
          CHK(check_range(o.i[0], o.i[1], "lincomb dst"));
          if (o.stage != 1) return fail(SSN_EUNSUPPORTED, "lincomb operators belong to the per-timestep core");
          if (o.i[2] < 0 || o.i[3] < 0 || o.i[3] >= m->n_buffers || o.i[4] < 0 || o.i[4] >= m->n_buffers) return fail(SSN_EINVAL, "lincomb term buffers out of range");
          const ssn_buffer_desc& sb = m->buffers[o.i[3]]; const ssn_buffer_desc& ab = m->buffers[o.i[4]];
          if (sb.kind != SSN_BUF_I32 || ab.kind != SSN_BUF_REAL || sb.count != o.i[2] || ab.count != o.i[2]) return fail(SSN_EINVAL, "lincomb term buffers: int32 offsets and real coefficients of n_terms elements each");
          for (int64_t q = 0; q < o.i[2]; ++q) CHK(check_range(((const int32_t*)sb.data)[q], o.i[1], "lincomb src"));
          break;
        }
        default: return fail(SSN_EINVAL, "unknown operator kind %d", o.kind);
      }
    }
    CHK(read_taps(m));
    CHK(read_drives(m));
    // uploads
    for (int i = 0; i < m->n_buffers; ++i) {
      Buf& b = bufs[i];
      if (b.kind == SSN_BUF_TAPS || b.kind == SSN_BUF_DRIVES) continue;       // (host-side records: read_taps, read_drives)
      if (b.kind == SSN_BUF_I32) {
        CHK(dupload((int32_t**)&b.d, (const int32_t*)m->buffers[i].data, b.count));
      } else {
        const int64_t elems = b.dec_DP ? (int64_t)b.dec_K * b.ld * b.dec_DP : (b.transposed ? b.cols * b.ldt : b.rows * b.ld);
        CHK(dmalloc((T**)&b.d, elems * (int64_t)sizeof(T)));
        CHK(upload_buf(b, (const double*)m->buffers[i].data));
        if (b.keep) b.host.assign((const double*)m->buffers[i].data, (const double*)m->buffers[i].data + b.count);
      }
    }
    CHK(upload(sig_init.data(), sig, 1, n_sig, n_sig));
    CHK(dzeros(&d_ctx, 1));
    // tables and probes
    tables.assign(m->n_tables, ssn::TableSlot{nullptr, nullptr, 0, 0, 0, 0});
    table_rows.resize((size_t)m->n_tables);
    table_idx.resize((size_t)m->n_tables);
    staged.resize((size_t)m->n_tables);
    CHK(dupload(&d_tables, tables));
    probes.assign(m->probes, m->probes + m->n_probes);
    for (auto& p : probes) {
      if (p.every < 1) return fail(SSN_EINVAL, "probe 'every' must be >= 1");
      CHK(check_range(p.src, p.width, "probe"));
    }
    pslots.assign(m->n_probes, ssn::ProbeSlot{nullptr, 1, 0, 0});
    probe_store.resize((size_t)m->n_probes);
    for (int i = 0; i < m->n_probes; ++i) pslots[i].every = probes[i].every;
    CHK(dupload(&d_pslots, pslots));
    exchange.assign(m->exchange, m->exchange + (m->n_exchange > 0 ? m->n_exchange : 0));
    phased = !exchange.empty();
    for (auto& r : exchange) CHK(check_range(r.lo, r.hi - r.lo, "exchange"));
    // time-batched stages
    bool has_batched_stage = false;
    for (int i = 0; i < m->n_ops; ++i) has_batched_stage = has_batched_stage || m->ops[i].stage != 1;
    for (auto& p : probes) has_batched_stage = has_batched_stage || p.stage != 1;
    batched_mask.assign((size_t)n_sig, 0);
    if (has_batched_stage && phased) return fail(SSN_EINVAL, "a neuron-sharded model is stepped whole (build it unstaged)");
    if (has_batched_stage) {
      // default: 1024 timesteps per block while the block buffer stays under 256 MiB, else 256
      block = m->block_steps > 0 ? m->block_steps : ((int64_t)1025 * n_sig * (int64_t)sizeof(T) <= (256ll << 20) ? 1024 : 256);
      CHK(dmalloc(&bsig, (int64_t)(block + 1) * n_sig * (int64_t)sizeof(T)));
      CHK(init_bsig());
      pre_to_core.assign(m->pre_to_core, m->pre_to_core + m->n_pre_to_core);
      core_to_post.assign(m->core_to_post, m->core_to_post + m->n_core_to_post);
      for (auto& r : pre_to_core) CHK(check_range(r.lo, r.hi - r.lo, "pre->core boundary"));
      for (auto& r : core_to_post) CHK(check_range(r.lo, r.hi - r.lo, "core->post boundary"));
    }
    // default: 64 timesteps per step graph where the time-batched blocks hold whole graphs (the software-pipelined round plan
    // fills and drains once per graph: SLAM config 3 106.3 us per timestep at 16, 105.9 at 32, 104.5 at 64 - round 4), else 16
    steps_per_graph = m->steps_per_graph != 0 ? m->steps_per_graph : ((block == 0 || block % 64 == 0) ? 64 : 16);
    if (steps_per_graph > 128) return fail(SSN_EINVAL, "steps_per_graph %d: at most 128 (a glue block carries its timestep offset in 8 signed bits)", steps_per_graph);
    CHK(drive_tables());
    CHK(plan(m));
    CHK(capture());
    HIPCHK(hipStreamSynchronize(stream));
    return SSN_OK;
  }

  // ---- planning ---------------------------------------------------------------------------
  ssn::NeuronParams<T> neuron_params(int64_t type, const double* f) const {
    ssn::NeuronParams<T> np;
    np.type = (int)type; np.dt = (T)dt; np.tau_rc = (T)f[0]; np.tau_ref = (T)f[1]; np.min_voltage = (T)f[2];
    return np;
  }

  void ens_chunking(ssn::EnsArgs<T>& a, int min_wgs = 4096) {
    // whole 256-thread sweeps per workgroup; keep >= ~4096 workgroups chip-wide while sweeps can grow (2048 inside a
    // round's grid, where other operators fill the chip as well: two sweeps per workgroup - the second streams in under
    // the first one's decoder gather - measured 148 -> 144 us per timestep at SLAM config 3)
    const int n_vec = a.n_pad / VW;
    int sweeps = 1;
    const int max_sweeps = (n_vec + 255) / 256;
    while (sweeps < max_sweeps && (int64_t)a.K * ((n_vec + 256 * (sweeps + 1) - 1) / (256 * (sweeps + 1))) >= min_wgs) ++sweeps;
    if (opt.ens_sweeps != PlanOptions::UNSET) sweeps = std::max(1, std::min(max_sweeps, opt.ens_sweeps));   // tuning knob
    a.chunk_vec = 256 * sweeps;
    a.P = (n_vec + a.chunk_vec - 1) / a.chunk_vec;
  }

  void fill_ens_args(const ssn_op_desc& o, const TapSet* ts, const DriveSet* ds, ssn::EnsArgs<T>& a) {
    a = ssn::EnsArgs<T>{};
    a.K = (int)o.i[1]; a.n = (int)o.i[2]; a.din = (int)o.i[3]; a.dout = (int)o.i[4];
    a.n_pad = (int)bufs[o.i[5]].ld;
    a.enc = (const T*)bufs[o.i[5]].d; a.bias = (const T*)bufs[o.i[6]].d; a.dec = (const T*)bufs[o.i[7]].d;
    a.V = (T*)bufs[o.i[9]].d; a.R = (T*)bufs[o.i[10]].d;
    a.sig = sig; a.x_off = o.i[0];
    a.np = neuron_params(o.i[11], o.f);
    a.xrows = nullptr; a.n_sig = n_sig; a.ctx = d_ctx; a.n_rec = 0;
    a.fast = ens_fast(o) ? (ens_sparse(o) ? 1 : 2) : 0;
    a.defer = 0; a.sub = 0; a.partials_stride = 0;
    if (ts) { a.tap = ts->d_tab; a.tap_amp = (T)ts->amp; a.tap_sig = sig; a.tap_rows = nullptr; }
    if (ds) { a.drv_m = ds->rec.m; a.drv_w = (const T*)bufs[ds->rec.w_buf].d; a.drv_src = ds->d_tab; }
    ens_chunking(a);
  }

  // FFT plan of a DFT-structured matvec: route and tables come from ssn_fft_plan.hpp; the simulator's own part is the cache of
  // uploaded tables, the kernel's arguments and the SSN_DEBUG_PLAN listing.  N = 0 when no route fits - the matrix is used then.
  // Injective key of a table: what it is (kind) and every size its contents depend on - a network with circular convolutions
  // of two different lengths must never be handed the other length's table.
  enum { DK_TWIDDLE = 1, DK_CHIRP = 2, DK_CHIRP_SPECTRUM = 3, DK_CHIRP_SPECTRUM_INPLACE = 4, DK_DFT4_G1 = 5, DK_DFT4_G2 = 6 };
  static int64_t dft_key(int kind, int a, int b = 0) { return ((int64_t)kind << 56) | ((int64_t)(uint32_t)a << 28) | (int64_t)(uint32_t)b; }
  // the table behind a key, made (make() -> host vector) and uploaded the first time it is asked for
  template <typename P, typename Make>
  int dft_table(int64_t key, Make make, const P** out) {
    for (auto& t : dft_tables) if (t.first == key) { *out = (const P*)t.second; return SSN_OK; }
    const auto h = make();
    static_assert(sizeof(h[0]) == sizeof(P), "a table is uploaded as it lies on the host");
    P* d = nullptr;
    CHK(dupload(&d, (const P*)h.data(), (int64_t)h.size()));
    dft_tables.push_back({key, (float2*)d});
    *out = d;
    return SSN_OK;
  }
  int plan_dft(const ssn_op_desc& o, ssn::DftArgs* a) {
    namespace fft = ssn::fft;
    const int kind = (int)o.i[6];
    const int d = kind == 5 ? (int)o.i[2] : (int)o.i[3];
    *a = ssn::DftArgs{};
    if (d < 8) return SSN_OK;
    fft::Route r;
    // opt-in (round 3, measured slower than the Stockham passes as built - DESIGN.md): the four-step transform on the matrix cores
    if (opt.has(SSN_PLAN_FOUR_STEP_FFT)) r = fft::plan_four_step(d, kind == 5);
    if (!r) r = fft::plan_stockham(d, !opt.dft_no_inplace);
    if (!r) return SSN_OK;
    CHK(dft_table(dft_key(DK_TWIDDLE, r.L), [&] { return fft::twiddles(r.L); }, &a->tw));
    if (r.M > 0) {      // (the spectrum depends on d, M and the engine)
      CHK(dft_table(dft_key(DK_CHIRP, d), [&] { return fft::chirp(d); }, &a->chirp));
      CHK(dft_table(dft_key(r.inplace ? DK_CHIRP_SPECTRUM_INPLACE : DK_CHIRP_SPECTRUM, d, r.M),
                    [&] { return fft::chirp_spectrum(d, r.M, r.inplace ? &r.radix : nullptr); }, &a->fb));
    }
    if (r.N1 > 0) {
      CHK(dft_table(dft_key(DK_DFT4_G1, r.N1, r.N2), [&] { return fft::dft4_matrix(r.N1); }, &a->g1));
      CHK(dft_table(dft_key(DK_DFT4_G2, r.N1, r.N2), [&] { return fft::dft4_matrix(r.N2); }, &a->g2));
    }
    a->src = (const float*)(sig + o.i[1]); a->dst = (float*)(sig + o.i[0]); a->N = d; a->kind = kind; a->set = (int)o.i[5];
    a->M = r.M; a->inplace = r.inplace; a->N1 = r.N1; a->N2 = r.N2; a->nr = (int)r.radix.size();
    for (size_t i = 0; i < r.radix.size(); ++i) a->radix[i] = r.radix[i];
    list_dft(*a);
    return SSN_OK;
  }
  // SSN_DEBUG_PLAN: what plan_dft planned, one line per transform (the caller may still keep the matrix: M >= 2048)
  void list_dft(const ssn::DftArgs& a) const {
    if (!opt.debug_plan) return;
    fprintf(stderr, "[ssn] dft kind %d N %d M %d inplace %d split %dx%d radices", a.kind, a.N, a.M, a.inplace, a.N1, a.N2);
    for (int i = 0; i < a.nr; ++i) fprintf(stderr, " %d", a.radix[i]);
    fprintf(stderr, "\n");
  }

  // Neuron order for the whole-block kernel (f32).  k_ens_block leaves out the spike-time arithmetic and the decode of a
  // (wave, round) slot - 64 lanes x SSN_BLOCK_IL neuron pairs - in which no neuron spikes (ssn_block.hpp).  With neurons in
  // sampling order some neuron of every slot always spikes; so the neurons of each ensemble are dealt to the slots by WHEN they
  // can fire.  For the oscillator ensembles (reference pathintegration.py:162-166: 3-D, state on a circle in the plane of the
  // first two dimensions, third dimension the frequency input) neuron i is driven above threshold while
  //   rho_i cos(theta - phi_i) > 1 - bias_i      (rho_i, phi_i: its scaled encoder in that plane; theta: the oscillator's phase)
  // i.e. always (class 0), never (class 2), or for theta within alpha_i = acos((1 - bias_i) / rho_i) of phi_i (class 1).  Class 1
  // is cut into bands of similar alpha and sorted by phi inside a band: a slot then holds neurons of one sector and falls
  // silent when the phase is elsewhere.  Any order is a valid order - sums over an ensemble's neurons do not depend on it beyond
  // rounding - so the heuristic only decides how often the shortcut applies (other 3-D ensembles: rarely, harmlessly).  The
  // permutation lives in the buffers' upload / download (Buf::perm): callers keep seeing their own order.
  int reorder_block_neurons(const ssn_model_desc* m, const ssn_op_desc& eo, int nthr, int npt) {
    const int64_t K = eo.i[1], n = eo.i[2], din = eo.i[3], dout = eo.i[4];
    if (din != 3 || n < 256) return SSN_OK;
    const double* enc = (const double*)m->buffers[eo.i[5]].data;        // [K][din][n]
    const double* bias = (const double*)m->buffers[eo.i[6]].data;       // [K][n]
    // positions of the ensemble's row in slot order: slot (round j, wave w) = positions of the groups j * IL ... j * IL + IL - 1
    // at the wave's 128 columns, group after group (neuron index of (group g, thread t, component c) = (g * nthr + t) * 2 + c)
    const int ng = npt / 2, il = std::min<int>(SSN_BLOCK_IL, ng), waves = nthr / 64;
    std::vector<int32_t> pos;
    pos.reserve((size_t)n);
    for (int j = 0; j * il < ng; ++j)
      for (int w = 0; w < waves; ++w)
        for (int u = 0; u < il && j * il + u < ng; ++u)
          for (int q = 0; q < 128; ++q) {
            const int64_t p = ((int64_t)(j * il + u) * nthr + w * 64) * 2 + q;
            if (p < n) pos.push_back((int32_t)p);
          }
    if ((int64_t)pos.size() != n) return SSN_OK;                        // (a variant this layout does not describe: keep the order)
    auto perm = std::make_shared<std::vector<int32_t>>((size_t)(K * n));
    struct Key { int cls; double a, phi; int32_t i; };
    std::vector<Key> keys((size_t)n);
    const int slot = 128 * il;
    for (int64_t k = 0; k < K; ++k) {
      const double* e0 = enc + (k * din + 0) * n; const double* e1 = enc + (k * din + 1) * n; const double* b = bias + k * n;
      int n1 = 0;
      for (int64_t i = 0; i < n; ++i) {
        const double rho = std::hypot(e0[i], e1[i]), mth = 1.0 - b[i];
        Key& q = keys[(size_t)i];
        q.i = (int32_t)i; q.phi = std::atan2(e1[i], e0[i]);
        if (!(rho > 0.0) || mth >= rho) { q.cls = 2; q.a = mth - rho; }
        else if (mth <= -rho) { q.cls = 0; q.a = 0.0; }
        else { q.cls = 1; q.a = std::acos(mth / rho); ++n1; }
      }
      // class 0 | class 1 by descending alpha | class 2 by how far below threshold
      std::sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) {
        if (x.cls != y.cls) return x.cls < y.cls;
        if (x.cls == 1 && x.a != y.a) return x.a > y.a;
        if (x.cls == 2 && x.a != y.a) return x.a < y.a;
        return x.i < y.i;
      });
      // bands of class 1: whole slots each, about four bands; inside a band by phi
      size_t lo = 0;
      while (lo < keys.size() && keys[lo].cls == 0) ++lo;
      const size_t hi = lo + (size_t)n1;
      const size_t band = std::max<size_t>(slot, ((size_t)n1 / 4 + slot - 1) / slot * slot);
      for (size_t s0 = lo; s0 < hi; s0 += band)
        std::sort(keys.begin() + (long)s0, keys.begin() + (long)std::min(hi, s0 + band), [](const Key& x, const Key& y) {
          return x.phi != y.phi ? x.phi < y.phi : x.i < y.i;
        });
      int32_t* pk = perm->data() + k * n;
      for (int64_t r = 0; r < n; ++r) pk[pos[(size_t)r]] = keys[(size_t)r].i;
    }
    struct Target { int64_t id; int rows; };
    for (const Target t : {Target{eo.i[5], (int)din}, Target{eo.i[6], 1}, Target{eo.i[7], (int)dout}, Target{eo.i[9], 1}, Target{eo.i[10], 1}}) {
      Buf& b = bufs[(size_t)t.id];
      if (b.cols != n) return fail(SSN_EINVAL, "ensemble array buffer %lld has %lld columns, expected %lld", (long long)t.id, (long long)b.cols, (long long)n);
      b.perm = perm; b.perm_rows = t.rows;
      if (b.packed == 2) continue;                                      // (the refractory view of the voltage buffer: no storage of its own to re-upload)
      CHK(upload_buf(b, (const double*)m->buffers[t.id].data));
    }
    return SSN_OK;
  }

  // Taps of the whole-block kernel: which workgroups have one (tap_slot[k], -1: none) and, per tapped ensemble, the
  // destination signal of every column of its row in the DEVICE's neuron order (-1: not tapped) - the order may be a
  // permutation of the caller's (reorder_block_neurons), so the kernel looks the destination up instead of computing it.
  int block_taps(const ssn_op_desc& eo, const TapSet* ts) {
    if (!ts) return SSN_OK;
    const int64_t K = eo.i[1], n = eo.i[2], row = blk.n_pad;
    const Buf& eb = bufs[(size_t)eo.i[5]];
    std::vector<int> slot((size_t)K, -1), col(ts->list.size() * (size_t)row, -1);
    for (size_t q = 0; q < ts->list.size(); ++q) {
      const ssn_tap_desc& t = ts->list[q];
      slot[(size_t)t.k] = (int)q;
      for (int64_t c = 0; c < n; ++c) {
        const int64_t orig = eb.perm ? (*eb.perm)[(size_t)(t.k * n + c)] : c;
        if (orig >= t.first && orig < t.first + t.count) col[q * (size_t)row + (size_t)c] = (int)(t.dst + orig - t.first);
      }
    }
    int* d_slot = nullptr; int* d_col = nullptr;
    CHK(dupload(&d_slot, slot));
    CHK(dupload(&d_col, col));
    blk.tap_slot = d_slot; blk.tap_col = d_col; blk.tap_amp = (T)ts->amp;
    return SSN_OK;
  }

  // Core stage == one recurrent ensemble array (the path integrator's VCO array): x assembled in the
  // kernel prologue, decoded rows / synapse update / hand-off / step counter in one barrier-free finish
  // kernel.  *fused stays false (and nothing is planned) when the core does not have that shape.
  int try_fused_core(const ssn_model_desc* m, bool* fused) {
    *fused = false;
    if (!bsig) return SSN_OK;
    for (auto& p : probes) if (p.stage == 1) return SSN_OK;
    int ens_i = -1;
    std::vector<int> axpys, lows;
    for (int i = 0; i < m->n_ops; ++i) {
      const ssn_op_desc& o = m->ops[i];
      if (o.stage != 1) continue;
      if (o.kind == SSN_OP_ENSARRAY) { if (ens_i >= 0) return SSN_OK; ens_i = i; }
      else if (o.kind == SSN_OP_AXPY && o.i[3] == 0) axpys.push_back(i);
      else if (o.kind == SSN_OP_LOWPASS) lows.push_back(i);
      else return SSN_OK;
    }
    if (ens_i < 0 || axpys.size() > 4) return SSN_OK;
    const ssn_op_desc& eo = m->ops[ens_i];
    const int64_t K = eo.i[1], din = eo.i[3], dout = eo.i[4];
    const int64_t x0 = eo.i[0], x1 = eo.i[0] + K * din;
    auto inside = [](int64_t lo, int64_t hi, const std::vector<ssn_range>& rs) {
      for (auto& r : rs) if (lo >= r.lo && hi <= r.hi) return true;
      return false;
    };
    if (!inside(x0, x1, pre_to_core)) return SSN_OK;
    for (int i : axpys) {                       // recurrent terms must land inside pre-stage-provided inputs
      const ssn_op_desc& o = m->ops[i];
      if (!inside(o.i[0], o.i[0] + o.i[2], pre_to_core)) return SSN_OK;
    }
    // drive columns: the fused prologue reads their scalars from the timestep's block row - every source must be a pre-stage
    // signal that no operator of the core adds to (the recurrent terms are folded into x only)
    const TapSet* const taps = taps_of(ens_i);
    const DriveSet* const drv = drives_of(ens_i);
    if (drv)
      for (int32_t sx : drv->src) {
        if (sx < 0) continue;
        if (!inside(sx, sx + 1, pre_to_core)) return SSN_OK;
        for (int i : axpys) if (sx >= m->ops[i].i[0] && sx < m->ops[i].i[0] + m->ops[i].i[2]) return SSN_OK;
        for (int i : lows) if (sx >= m->ops[i].i[0] && sx < m->ops[i].i[0] + m->ops[i].i[2]) return SSN_OK;
      }
    const int32_t* didx = (const int32_t*)m->buffers[eo.i[8]].data;
    std::vector<int> row_of((size_t)n_sig, -1);
    for (int64_t j = 0; j < K * dout; ++j) row_of[(size_t)didx[j]] = (int)j;   // padded rows share a trash slot: harmless
    std::vector<int> lp_state((size_t)(K * dout), -1);
    std::vector<double> lp_a((size_t)(K * dout), 0.0), lp_b((size_t)(K * dout), 0.0);
    std::vector<unsigned char> rowout((size_t)(K * dout), 0);
    for (int i : lows) {
      const ssn_op_desc& o = m->ops[i];
      for (int64_t e = 0; e < o.i[2]; ++e) {
        const int row = row_of[(size_t)(o.i[1] + e)];
        if (row < 0) {
          // no local row feeds this filter input (VCO owned by another rank): input and state stay 0,
          // provided nothing else writes that signal
          if (inside(o.i[1] + e, o.i[1] + e + 1, pre_to_core) || sig_init[(size_t)(o.i[1] + e)] != 0.0) return SSN_OK;
          continue;
        }
        if (lp_state[(size_t)row] >= 0) return SSN_OK;
        lp_state[(size_t)row] = (int)(o.i[0] + e);
        lp_a[(size_t)row] = o.f[0];
        lp_b[(size_t)row] = (1.0 - o.f[0]) * o.f[1];
      }
    }
    for (auto& r : core_to_post)
      for (int64_t e = r.lo; e < r.hi; ++e) {
        const int row = row_of[(size_t)e];
        if (row >= 0) rowout[(size_t)row] = 1;      // (elements no local row writes stay at their initial value)
      }
    // ---- can the finish be deferred into the next step's prologue?  every recurrent term must read a
    //      filter state owned by a row of the SAME ensemble (ens_k -> Lowpass -> ens_k), one term per input
    bool defer = !opt.has(SSN_PLAN_SEPARATE_FINISH);        // decided below: only worth it in the latency-bound regime (few workgroups)
    std::vector<int> xrow((size_t)(K * din), -1), lp_has((size_t)(K * dout), 0);
    std::vector<double> xalpha((size_t)(K * din), 0.0);
    {
      std::vector<int> owner((size_t)n_sig, -1);
      for (int64_t j = 0; j < K * dout; ++j)
        if (lp_state[(size_t)j] >= 0) { owner[(size_t)lp_state[(size_t)j]] = (int)j; lp_has[(size_t)j] = 1; }
      // filter states whose input no row writes (dropped all-zero decoder rows, other ranks' VCOs) stay 0
      std::vector<unsigned char> dead_zero((size_t)n_sig, 0);
      for (int i : lows) {
        const ssn_op_desc& o = m->ops[i];
        for (int64_t e = 0; e < o.i[2]; ++e) {
          const int64_t st = o.i[0] + e, src = o.i[1] + e;
          if (row_of[(size_t)src] < 0 && sig_init[(size_t)st] == 0.0 && sig_init[(size_t)src] == 0.0 &&
              !inside(src, src + 1, pre_to_core)) dead_zero[(size_t)st] = 1;
        }
      }
      for (int i : axpys) {
        const ssn_op_desc& o = m->ops[i];
        for (int64_t e = 0; e < K * din && defer; ++e) {
          const int64_t xi = x0 + e;
          if (xi < o.i[0] || xi >= o.i[0] + o.i[2]) continue;
          const int64_t st = o.i[1] + (xi - o.i[0]);
          const int row = owner[(size_t)st];
          if (row < 0 && dead_zero[(size_t)st]) continue;               // adds exactly 0
          if (row < 0 || row / dout != e / din || xrow[(size_t)e] >= 0) defer = false;
          else { xrow[(size_t)e] = (int)(row % dout); xalpha[(size_t)e] = o.f[0]; }
        }
      }
    }
    // the filter tables of either plan: per decoded row its filter state, coefficients and hand-off flag; with_x: per input
    // the row whose state feeds it back, and that term's gain
    const int64_t nr = K * dout;
    struct FilterTabs { int* lp = nullptr; T* a = nullptr; T* b = nullptr; unsigned char* ro = nullptr; int* xrow = nullptr; T* xalpha = nullptr; };
    auto filter_tables = [&](FilterTabs& t, bool with_x) -> int {
      CHK(dupload(&t.lp, lp_state));
      CHK(dmalloc(&t.a, nr * (int64_t)sizeof(T)));
      CHK(dmalloc(&t.b, nr * (int64_t)sizeof(T)));
      CHK(dupload(&t.ro, rowout));
      CHK(upload(lp_a.data(), t.a, 1, nr, nr));
      CHK(upload(lp_b.data(), t.b, 1, nr, nr));
      if (!with_x) return SSN_OK;
      CHK(dupload(&t.xrow, xrow));
      CHK(dmalloc(&t.xalpha, K * din * (int64_t)sizeof(T)));
      CHK(upload(xalpha.data(), t.xalpha, 1, K * din, K * din));
      return SSN_OK;
    };
    // ---- plan A: the ensembles are independent inside a block -> one k_ens_block launch per block -----
    int blk_threads = 0, blk_tpb = 0, blk_npt = 0, blk_lds = 0;
    // (One workgroup steps one ensemble.  Splitting an ensemble over P workgroups that exchange partial sums through L2
    //  every timestep was built and measured in round 1 - 3.3 us per timestep at P = 2 and 3.6 at P = 4 against 2.95 for
    //  one workgroup on 127- / 64-VCO shards: a cross-CU round trip costs ~1.6 us, more than halving the neuron work
    //  saves - and removed in round 2: DESIGN.md section 5.)
    // Split ensembles (flag 1073741824; f32, dout <= 4): when the array has fewer ensembles than the GPU has CUs - a 4- or
    // 8-GPU shard of config 2, a small model - P = 2 or 4 member workgroups step one ensemble and exchange their partial sums
    // every timestep (k_ens_block; the exchange costs 0.5 - 0.6 us per timestep, tools/xcd_exchange.hip).  All K * P
    // workgroups must be resident together, so P is only raised while K * P fits the CUs - and the caller only asks for
    // it when this process has the GPU to itself.
    int split_P = 1, n_member = 0;
    if (opt.has(SSN_PLAN_SPLIT_BLOCK) && sizeof(T) == 4 && dout <= 4) {
      hipDeviceProp_t prop;
      int n_cu = 256;
      if (hipGetDeviceProperties(&prop, device) == hipSuccess) n_cu = prop.multiProcessorCount;
      if (opt.block_split_cus != PlanOptions::UNSET) n_cu = opt.block_split_cus;            // (tests: pretend the GPU is smaller / larger)
      const int64_t n_ens = eo.i[2];
      for (int cand : {4, 2}) {
        if (K * cand <= n_cu && n_ens / cand >= 1024) { split_P = cand; break; }
      }
      { const int q = opt.block_split; if (q == 1 || q == 2 || q == 4 || q == 8) split_P = q; }
      if (split_P > 1) n_member = (int)(((n_ens + split_P - 1) / split_P + 3) / 4 * 4);
    }
    // (a driven array is not eligible: k_ens_block has no drive columns)
    if (defer && !drv && !opt.has(SSN_PLAN_NO_BLOCK_KERNEL) && ens_fast(eo) && (sizeof(T) == 8 || (dt <= 0.05 * eo.f[0] && eo.f[1] >= dt && ssn::lif_affine_kappa((double)(T)dt, (double)(T)eo.f[0], (double)(T)eo.f[1]) >= 4.0)) &&
        ssn::ens_block_supported<T>((int)din, (int)dout, split_P > 1 ? n_member : (int)eo.i[2], opt.block_variant.v, &blk_threads, &blk_tpb, &blk_npt, &blk_lds)) {
      FilterTabs ft;
      CHK(filter_tables(ft, true));
      ssn::EnsArgs<T> ea;
      fill_ens_args(eo, taps, drv, ea);
      blk = ssn::BlockArgs<T>{};
      blk.enc = ea.enc; blk.bias = ea.bias; blk.dec = ea.dec; blk.S = ea.V;
      blk.xrows = bsig; blk.bsig = bsig; blk.sig = sig; blk.sig_w = sig;
      blk.didx = (const int*)bufs[eo.i[8]].d; blk.lp_state = ft.lp; blk.lp_a = ft.a; blk.lp_b = ft.b;
      blk.xrow = ft.xrow; blk.xalpha = ft.xalpha; blk.rowout = ft.ro;
      blk.n_sig = n_sig; blk.x_off = eo.i[0];
      blk.K = ea.K; blk.n = ea.n; blk.n_pad = ea.n_pad; blk.din = ea.din; blk.dout = ea.dout;
      blk.B = 0; blk.row0 = 1; blk.threads = blk_threads; blk.tpb = blk_tpb; blk.npt = blk_npt; blk.enc_lds = blk_lds;
      blk.dec_neuron_major = ea.fast == 1 ? 1 : 0;
      blk.np = ea.np;
      blk.P = split_P; blk.n_member = n_member; blk.xslots = nullptr; blk.xerr = nullptr;
      {
        unsigned long long* d_ss = nullptr;
        CHK(dzeros(&d_ss, 2));
        blk.slot_stats = d_ss;
      }
      if (split_P > 1) {
        unsigned int* d_x = nullptr; int* d_e = nullptr;
        CHK(dmalloc(&d_x, (int64_t)3 * K * 64 * 4));
        CHK(dzeros(&d_e, 4));
        blk.xslots = d_x; blk.xerr = d_e;
      }
      dom_units = (int64_t)ea.K * ea.n * block;
      dom_bytes = (double)dom_units * (ea.din + ea.dout + 5) * sizeof(T);
      *fused = fused_core = fused_block = true;
      // (only worth anything with a kernel built with SSN_BLOCK_SKIP = 1 or 2 - both measured slower than the plain loop, round 4 -
      //  so the neuron order is the caller's unless SSN_BLOCK_SORT=1 asks for the slot order)
      if (sizeof(T) == 4 && split_P == 1 && opt.block_sort)
        CHK(reorder_block_neurons(m, eo, blk_npt == 2 ? blk_threads : blk_tpb, blk_npt));
      return block_taps(eo, taps);
    }
    // ---- plan B: [k_ensarray (fused prologue), k_ens_finish] ------------------------------------------
    Item it; it.type = IT_ENS;
    fill_ens_args(eo, taps, drv, it.ens);
    it.taps = taps; it.drv = drv;
    ssn::EnsArgs<T>& a = it.ens;
    a.xrows = bsig;
    if (a.tap) a.tap_rows = bsig;      // (a fused core has no hand-off operator: the kernel writes the post stage's rows itself)
    if (drv) a.drv_src = drv->d_tab_rows;      // (no row-in operator either: pre-stage sources are read from the block row)
    // measured on MI355X (tools/bench_shard.py): 5080 workgroups (config 2 on one GPU) 35.4 us/step with the
    // separate finish kernel vs 37.4 deferred; 2540 / 1270 / 640 workgroups (2 / 4 / 8-GPU shards) 24.5 / 15.8 /
    // 13.1 vs 22.0 / 12.5 / 9.4 deferred
    // (one process, full size: 36.6 us/step deferred vs 37.4 with the finish kernel -> deferred whenever it applies)
    for (int i : axpys) {
      const ssn_op_desc& o = m->ops[i];
      a.rec_dst[a.n_rec] = o.i[0]; a.rec_src[a.n_rec] = o.i[1]; a.rec_len[a.n_rec] = o.i[2]; a.rec_alpha[a.n_rec] = (T)o.f[0];
      ++a.n_rec;
    }
    a.partials_stride = (int64_t)a.K * a.P * a.dout;
    CHK(dzeros(&a.partials, 2 * a.partials_stride));
    it.dominant = true;
    dom_units = (int64_t)a.K * a.n;
    dom_bytes = (double)dom_units * (a.din + a.dout + 5) * sizeof(T);
    Item fi; fi.type = IT_FINISH;
    ssn::FinishArgs<T>& f = fi.fin;
    f = ssn::FinishArgs<T>{};
    FilterTabs ft;                        // (the feedback rows: only the deferred finish reads them)
    CHK(filter_tables(ft, defer));
    unsigned int* d_ticket = nullptr;
    CHK(dzeros(&d_ticket, 16));
    f.partials = a.partials; f.didx = (const int*)bufs[eo.i[8]].d; f.lp_state = ft.lp; f.lp_a = ft.a; f.lp_b = ft.b;
    f.rowout = ft.ro; f.sig = sig; f.bsig = bsig; f.n_sig = n_sig; f.ctx = d_ctx; f.ticket = d_ticket;
    f.K = a.K; f.P = a.P; f.dout = a.dout; f.n_blocks = (int)((nr + 255) / 256);
    f.mode = 0; f.fstate = nullptr; f.partials_stride = a.partials_stride; f.lp_has = nullptr;
    if (defer) {
      int* d_has = nullptr; T* d_fstate = nullptr;
      CHK(dupload(&d_has, lp_has));
      CHK(dzeros(&d_fstate, 2 * nr));
      a.defer = 1; a.sub = 0; a.didx = f.didx; a.lp_has = d_has; a.lp_a = ft.a; a.lp_b = ft.b; a.fstate = d_fstate;
      a.xrow = ft.xrow; a.xalpha = ft.xalpha; a.rowout = ft.ro; a.bsig = bsig; a.sig_w = sig;
      f.fstate = d_fstate; f.lp_has = d_has;
      fin_flush = f; fin_flush.mode = 1;
      fin_begin = f; fin_begin.mode = 2;
      items.push_back(it);
      *fused = fused_core = fused_defer = true;
      return SSN_OK;
    }
    items.push_back(it);
    items.push_back(fi);
    *fused = fused_core = true;
    // the batched stages are planned by plan(); nothing else runs per timestep
    return SSN_OK;
  }

  int plan(const ssn_model_desc* m) {
    bool fused = false;
    if (!opt.has(SSN_PLAN_NO_FUSED_CORE)) CHK(try_fused_core(m, &fused));
    std::vector<std::vector<MOp>> programs;   // programs in step order
    std::vector<int> item_prog;               // for IT_PROGRAM items: index into programs
    std::vector<MOp> cur;
    int prev_level = -1;
    bool force_barrier = false;
    // Element-wise micro operators are executed with element p of a range starting at `base` on thread
    // (p - base) mod 1024.  A dependency between two of them therefore needs no workgroup barrier when both map every
    // shared element to the same thread (equal range starts modulo 1024): program order inside the thread suffices.
    // (Here and for the grid-wide head below, an empty range that lies inside another one counts as touching it: keep_empty.)
    auto level_change_needs_barrier = [&](const MOp& op) -> bool {
      if (!kind_is(op.kind, ssn::MK_SAME_THREAD)) return true;
      std::vector<Rng> mine, theirs;
      micro_access(mine, op, false, true);
      for (size_t q = cur.size(); q-- > 0;) {             // operators since the last barrier
        if (!kind_is(cur[q].kind, ssn::MK_SAME_THREAD)) return true;
        theirs.clear();
        micro_access(theirs, cur[q], false, true);
        for (const Rng& x : mine)
          for (const Rng& y : theirs)
            if ((x.w || y.w) && x.lo < y.hi && y.lo < x.hi && ((x.lo - y.lo) % 1024) != 0) return true;
        if (cur[q].barrier) break;
      }
      return false;
    };
    auto push_micro = [&](MOp op, int level, bool exec_inserted) {
      if (cur.empty()) op.barrier = 0;
      else if (force_barrier || exec_inserted) op.barrier = 1;
      else if (level != prev_level) op.barrier = level_change_needs_barrier(op) ? 1 : 0;
      else op.barrier = 0;
      force_barrier = exec_inserted;
      prev_level = level;
      cur.push_back(op);
    };
    auto flush = [&]() {
      if (cur.empty()) return;
      Item it; it.type = IT_PROGRAM;
      item_prog.push_back((int)programs.size());
      programs.push_back(cur);
      items.push_back(it);
      cur.clear();
      force_barrier = false;
      prev_level = -1;
    };
    int64_t best_units = -1;
    int best_item = -1;
    int cur_phase = 0;
    for (auto& r : pre_to_core) {        // the pre stage's results for this timestep
      if (fused) break;
      MOp op{};
      op.kind = ssn::M_ROW_IN; op.dst = r.lo; op.len = r.hi - r.lo; op.p0 = bsig; op.i0 = n_sig; op.i1 = r.lo;
      push_micro(op, -10, false);
    }
    std::vector<std::pair<int, ssn::BatchOp<T>>> pre_sorted, post_sorted;
    std::vector<std::pair<MOp, int>> pending_reduce;
    auto drain_reduces = [&]() {
      bool first = true;
      for (auto& pr : pending_reduce) { push_micro(pr.first, pr.second, first); first = false; }
      pending_reduce.clear();
    };
    for (int i = 0; i < m->n_ops; ++i) {
      const ssn_op_desc& o = m->ops[i];
      MOp op{};
      const size_t items_before = items.size();
      if (phased && o.stage == 1 && o.phase != cur_phase) {      // the exchange: no program spans it
        if (o.phase < cur_phase) return fail(SSN_EINVAL, "operators of phase 0 after phase 1");
        flush();
        for (auto& it : items) if (it.phase < 0) it.phase = cur_phase;
        cur_phase = o.phase;
      }
      struct LevelTag { std::vector<Item>& v; size_t from; int level; ~LevelTag() { for (size_t q = from; q < v.size(); ++q) if (v[q].type != IT_PROGRAM && v[q].level < 0) v[q].level = level; } }
          level_tag{items, items_before, o.level};
      if (o.stage == 1 && !fused && !pending_reduce.empty() &&
          !(o.kind == SSN_OP_MATVEC && !is_micro(o) && bufs[o.i[4]].transposed && !opt.has(SSN_PLAN_NO_ITEM_BATCH)))
        drain_reduces();
      if (o.stage != 1) {
        ssn::BatchOp<T> b{};
        b.bsig = bsig; b.n_sig = n_sig; b.src_prev = o.src_prev ? 1 : 0;
        int64_t wlo = 0, wlen = 0;
        switch (o.kind) {
          case SSN_OP_FILL: b.kind = ssn::M_FILL; b.dst = o.i[0]; b.len = o.i[1]; b.a = (T)o.f[0]; wlo = o.i[0]; wlen = o.i[1]; break;
          case SSN_OP_TABLE: b.kind = ssn::M_TABLE; b.dst = o.i[0]; b.len = o.i[1]; b.p0 = d_tables + o.i[2];
            tables[o.i[2]].width = o.i[1]; wlo = o.i[0]; wlen = o.i[1]; break;
          case SSN_OP_AXPY: b.kind = o.i[3] ? ssn::M_AXPY_SET : ssn::M_AXPY_INC; b.dst = o.i[0]; b.src = o.i[1]; b.len = o.i[2];
            b.a = (T)o.f[0]; wlo = o.i[0]; wlen = o.i[2]; break;
          case SSN_OP_LOWPASS: b.kind = ssn::M_LOWPASS; b.dst = o.i[0]; b.src = o.i[1]; b.len = o.i[2];
            b.a = (T)o.f[0]; b.b = (T)((1.0 - o.f[0]) * o.f[1]); wlo = o.i[0]; wlen = o.i[2]; break;
          case SSN_OP_MATVEC: b.kind = o.i[5] ? ssn::M_MATVEC_SET : ssn::M_MATVEC_INC; b.dst = o.i[0]; b.src = o.i[1];
            b.len = o.i[2]; b.cols = (int)o.i[3]; b.ld = (int)bufs[o.i[4]].ld; b.p0 = bufs[o.i[4]].d; wlo = o.i[0]; wlen = o.i[2]; break;
          default: return fail(SSN_EUNSUPPORTED, "operator kind %d cannot run in a time-batched stage", o.kind);
        }
        for (int64_t j = wlo; j < wlo + wlen; ++j) batched_mask[(size_t)j] = 1;
        (o.stage == 0 ? pre_sorted : post_sorted).push_back({o.border, b});
        continue;
      }
      if (fused) continue;               // the core is [k_ensarray, k_ens_finish], planned above
      switch (o.kind) {
        case SSN_OP_FILL:
          op.kind = ssn::M_FILL; op.dst = o.i[0]; op.len = o.i[1]; op.a = (T)o.f[0];
          push_micro(op, o.level, false); break;
        case SSN_OP_TABLE:
          op.kind = ssn::M_TABLE; op.dst = o.i[0]; op.len = o.i[1]; op.p0 = d_tables + o.i[2];
          tables[o.i[2]].width = o.i[1];
          push_micro(op, o.level, false); break;
        case SSN_OP_AXPY:
          op.kind = o.i[3] ? ssn::M_AXPY_SET : ssn::M_AXPY_INC; op.dst = o.i[0]; op.src = o.i[1]; op.len = o.i[2]; op.a = (T)o.f[0];
          push_micro(op, o.level, false); break;
        case SSN_OP_LOWPASS:
          op.kind = ssn::M_LOWPASS; op.dst = o.i[0]; op.src = o.i[1]; op.len = o.i[2];
          op.a = (T)o.f[0]; op.b = (T)((1.0 - o.f[0]) * o.f[1]);
          push_micro(op, o.level, false); break;
        case SSN_OP_LINCOMB: {
          std::vector<ssn::LinTerm<T>> terms((size_t)o.i[2]);
          for (int64_t q = 0; q < o.i[2]; ++q)
            terms[(size_t)q] = ssn::LinTerm<T>{(long long)((const int32_t*)m->buffers[o.i[3]].data)[q], (T)((const double*)m->buffers[o.i[4]].data)[q]};
          ssn::LinTerm<T>* d_terms = nullptr;
          CHK(dupload(&d_terms, terms));
          lin_terms[(const void*)d_terms] = terms;
          op.kind = ssn::M_LINCOMB; op.dst = o.i[0]; op.len = o.i[1]; op.i0 = o.i[2]; op.p0 = d_terms;
          op.a = (T)o.f[0]; op.b = T(1); op.c = (T)o.f[1];
          push_micro(op, o.level, false); break;
        }
        case SSN_OP_GATE:
          op.kind = ssn::M_GATE; op.dst = o.i[0]; op.src = o.i[1]; op.len = o.i[2]; op.a = (T)o.f[0]; op.b = (T)o.f[1];
          push_micro(op, o.level, true); break;
        case SSN_OP_MATVEC: {
          const Buf& w = bufs[o.i[4]];
          ssn::DftArgs da{};
          // (a chirp-z transform of M >= 2048 points is two long FFTs on ONE workgroup: 16.5 us per launch at d = 1801 with the
          //  in-register radix-8 passes of round 3 (38.5 us with generic radix-16 butterflies) against ~7 us for its 26 MB matrix
          //  spread over the chip - measured on config 5: 266 us per timestep with the matrices, 288 - 295 with the FFT as a body
          //  of the round grid; the matrix is used for such a length unless flag 268435456 asks for the FFT)
          if (o.i[6] && sizeof(T) == 4 && !opt.has(SSN_PLAN_NO_FFT) && plan_dft(o, &da) == SSN_OK && da.N &&
              (da.M < 2048 || opt.has(SSN_PLAN_BLUESTEIN_FFT))) {
            // the matrix is a real-DFT map of a circular-convolution network: mixed-radix FFT instead of a GEMV
            flush();
            Item it; it.type = IT_DFT; it.dft = da;
            it.src = sig + o.i[1]; it.dst = sig + o.i[0]; it.rows = (int)o.i[2]; it.cols = (int)o.i[3];
            items.push_back(it);
            break;
          }
          if (is_micro(o)) {
            op.kind = o.i[5] ? ssn::M_MATVEC_SET : ssn::M_MATVEC_INC;
            op.dst = o.i[0]; op.src = o.i[1]; op.len = o.i[2]; op.i0 = o.i[3]; op.i1 = w.ld; op.p0 = w.d;
            push_micro(op, o.level, false);
          } else if (w.transposed) {
            // spike-sparse decoders: partial sums per spike-list chunk, reduced in the following program
            flush();
            int chunks = 32;
            const int rows_pad = (int)w.ldt;
            int seg = 0;
            if (std::find(seg_spikes.begin(), seg_spikes.end(), o.i[1]) != seg_spikes.end()) {
              const int n_seg = ((int)o.i[3] + 255) / 256;       // segments of 256 neurons, ~32 chunks
              const int max_chunks = std::max(1, opt.spmv_max_chunks);      // (A/B knob)
              seg = std::max(1, (n_seg + max_chunks - 1) / max_chunks);
              chunks = (n_seg + seg - 1) / seg;
            }
            T* partial = nullptr;
            CHK(dmalloc(&partial, (int64_t)chunks * rows_pad * (int64_t)sizeof(T)));
            Item it; it.type = IT_SPMV; it.Wm = (T*)w.d; it.src = sig + o.i[1]; it.dst = partial;
            it.rows = (int)o.i[2]; it.cols = (int)o.i[3]; it.ld = (int)w.ldt; it.n = chunks; it.seg = seg;
            for (auto& sl : spike_lists) if (sl.first == o.i[1]) { it.list = sl.second.first; it.count = sl.second.second; }
            {
              // the chunk reduction is deferred past any sparse products that follow directly (they read spike vectors,
              // never a reduction's output): the products then sit next to each other and share a launch, and their
              // reductions share one program
              items.push_back(it);
              MOp r{};
              r.kind = o.i[5] ? ssn::M_REDUCE_SET : ssn::M_REDUCE_INC; r.dst = o.i[0]; r.len = o.i[2]; r.i0 = chunks; r.i1 = rows_pad; r.p0 = partial;
              pending_reduce.push_back({r, o.level});
            }
          } else {
            flush();
            Item it; it.type = IT_MATVEC; it.Wm = (T*)w.d; it.src = sig + o.i[1]; it.dst = sig + o.i[0];
            it.rows = (int)o.i[2]; it.cols = (int)o.i[3]; it.ld = (int)w.ld; it.set = (int)o.i[5];
            items.push_back(it);
          }
          break;
        }
        case SSN_OP_ENSARRAY: {
          flush();
          Item it; it.type = IT_ENS;
          ssn::EnsArgs<T>& a = it.ens;
          it.taps = taps_of(i); it.drv = drives_of(i);
          fill_ens_args(o, it.taps, it.drv, a);
          ens_chunking(a, 2048);
          CHK(dmalloc(&a.partials, (int64_t)a.K * a.P * a.dout * (int64_t)sizeof(T)));
          const int64_t units = (int64_t)a.K * a.n;
          if (units > best_units) { best_units = units; best_item = (int)items.size(); }
          host_idx.push_back({bufs[o.i[8]].d, {(const int32_t*)m->buffers[o.i[8]].data, (int64_t)a.K * a.dout}});
          if (a.P == 1 && !opt.has(SSN_PLAN_ENS_PARTIALS)) {
            // one workgroup covers a whole ensemble (the 8128 product ensembles of 50 neurons): it writes the decoded
            // rows itself, no finish operator (and no program launch) behind the kernel
            a.direct = 1; a.didx = (const int*)bufs[o.i[8]].d; a.sig_w = sig;
            items.push_back(it);
            force_barrier = true;
            break;
          }
          items.push_back(it);
          MOp f{};
          f.kind = ssn::M_ENS_FINISH; f.len = (int64_t)a.K * a.dout; f.i0 = a.P; f.i1 = a.dout;
          f.p0 = a.partials; f.p1 = bufs[o.i[8]].d;
          push_micro(f, o.level, true);
          break;
        }
        case SSN_OP_NEURONS: {
          flush();
          Item it; it.type = IT_NEURONS; it.src = sig + o.i[0]; it.dst = sig + o.i[1]; it.n = (int)o.i[2];
          it.V = (T*)bufs[o.i[3]].d; it.R = (T*)bufs[o.i[4]].d; it.np = neuron_params(o.i[5], o.f); it.scalar = (T)o.f[3];
          bool feeds_sparse = false;     // does a spike-sparse decoder product read this ensemble's spikes?
          for (int j = 0; j < m->n_ops; ++j) {
            const ssn_op_desc& q = m->ops[j];
            if (q.kind == SSN_OP_MATVEC && q.stage == 1 && q.i[1] == o.i[1] && q.i[3] == o.i[2] && bufs[q.i[4]].transposed) feeds_sparse = true;
          }
          if (feeds_sparse && !opt.has(SSN_PLAN_SPMV_OWN_LIST)) {
            // segmented spike list: every 256-neuron workgroup of k_neurons leaves its spikes as an ordered index list
            const int n_seg = ((int)o.i[2] + 255) / 256;
            CHK(dmalloc(&it.list, (int64_t)n_seg * 256 * 4));
            CHK(dzeros(&it.count, (int64_t)n_seg + 16));
            spike_lists.push_back({o.i[1], {it.list, it.count}});
            seg_spikes.push_back(o.i[1]);
          }
          items.push_back(it);
          break;
        }
        case SSN_OP_PES: {
          flush();
          const Buf& w = bufs[o.i[0]];
          Item it; it.type = IT_PES; it.Wm = (T*)w.d; it.rows = (int)o.i[1]; it.cols = (int)o.i[2]; it.ld = (int)w.ld;
          it.aux0 = sig + o.i[3]; it.aux1 = sig + o.i[4]; it.scalar = (T)o.f[0];
          if (w.transposed) {   // neuron-major weights: W^T[c][r] += kappa * act[c] * err[r]
            it.rows = (int)o.i[2]; it.cols = (int)o.i[1]; it.ld = (int)w.ldt; it.aux0 = sig + o.i[4]; it.aux1 = sig + o.i[3];
          }
          items.push_back(it);
          break;
        }
        case SSN_OP_VOJA: {
          flush();
          const Buf& w = bufs[o.i[0]];
          Item it; it.type = IT_VOJA; it.Wm = (T*)w.d; it.rows = (int)o.i[1]; it.cols = (int)o.i[2]; it.ld = (int)w.ld;
          it.src = sig + o.i[3]; it.aux0 = sig + o.i[4]; it.aux1 = sig + o.i[5]; it.aux2 = (const T*)bufs[o.i[6]].d;
          it.scalar = (T)o.f[0];
          items.push_back(it);
          break;
        }
        case SSN_OP_CLEANUP: {
          // similarities S @ x into a scratch vector (k_matvec), then argmax + row gather in the next program
          flush();
          const Buf& w = bufs[o.i[4]];
          const int64_t grid_min_bytes = opt.grid_min_mb << 20;
          bool grid_route = sizeof(T) == 4 && o.i[5] > 0 && !opt.has(SSN_PLAN_NO_FACTORED_GRID) && o.i[2] * o.i[3] * (int64_t)sizeof(T) >= grid_min_bytes;
          // Round 4: a smaller grid (2-D, 10^4 rows: 40 MB of HBM stream per timestep at d = 1015) also goes through its factor
          // tables when the step runs as rounds - as bodies of the round grid (no MFMA product: 10^4 dot products of length 2K
          // from two L2-resident 100 x 2K tables), so nothing is launched on its own.  SSN_GRID_DOT_MIN_MB moves the threshold.
          const bool grid_dot = !grid_route && sizeof(T) == 4 && o.i[5] > 0 && !(opt.flags & (SSN_PLAN_NO_FACTORED_GRID | SSN_PLAN_NO_ROUNDS)) && o.i[2] < 65536 &&
                                o.i[10] * (int64_t)sizeof(T) <= 48 * 1024 &&
                                o.i[2] * o.i[3] * (int64_t)sizeof(T) >= (opt.grid_dot_min_mb << 20);
          grid_route = grid_route || grid_dot;
          // K-split of the grid product (partial products summed by the argmax's first stage): enough workgroups to hide latency
          int gsplit = grid_route && o.i[2] >= 65536 ? (int)std::min<int64_t>(4, std::max<int64_t>(1, o.i[10] / 448)) : 1;
          if (grid_route && o.i[2] >= 65536 && opt.grid_split != PlanOptions::UNSET) gsplit = std::max(1, std::min(8, opt.grid_split));
          for (int it2 = 0; it2 < 4; ++it2) {            // the split count the launcher's 32-column slabs actually produce
            const int kper = (((int)o.i[10] + gsplit - 1) / gsplit + 31) / 32 * 32;
            gsplit = ((int)o.i[10] + kper - 1) / kper;
          }
          T* scratch = nullptr;
          CHK(dmalloc(&scratch, o.i[2] * gsplit * (int64_t)sizeof(T)));
          Item it; it.type = IT_MATVEC; it.Wm = (T*)w.d; it.src = sig + o.i[1]; it.dst = scratch;
          it.rows = (int)o.i[2]; it.cols = (int)o.i[3]; it.ld = (int)w.ld; it.set = 1;
          if (grid_route) {
            // big sample grid (10^6 points in 3-D): similarities from the grid's factor tables - half spectrum of x
            // (k_matvec with the DFT rows), left operand (k_grid_lhs), one MFMA product - instead of streaming the
            // table; the table itself is only read for the winning row
            const Buf& fd = bufs[o.i[5] - 1]; const Buf& fl = bufs[o.i[6] - 1]; const Buf& fr = bufs[o.i[7] - 1];
            const int na = (int)o.i[8], nn = (int)o.i[9], k2 = (int)o.i[10];
            T* X = nullptr; T* A = nullptr;
            CHK(dmalloc(&X, k2 * (int64_t)sizeof(T)));
            CHK(dmalloc(&A, (int64_t)na * k2 * (int64_t)sizeof(T)));
            Item sx; sx.type = IT_MATVEC; sx.Wm = (T*)fd.d; sx.src = sig + o.i[1]; sx.dst = X;
            sx.rows = k2; sx.cols = (int)o.i[3]; sx.ld = (int)fd.ld; sx.set = 1;
            items.push_back(sx);
            Item sl; sl.type = IT_GRID_LHS; sl.src = X; sl.aux0 = (const T*)fl.d; sl.ld = (int)fl.ld; sl.dst = A;
            sl.rows = na; sl.cols = k2;
            items.push_back(sl);
            it.type = grid_dot ? IT_GRID_DOT : IT_GRID_GEMM; it.src = A; it.Wm = (T*)fr.d; it.ld = (int)fr.ld; it.rows = na; it.n = nn; it.cols = k2;
            it.seg = gsplit;
          }
          if (sizeof(T) == 8) {
            // parity mode: ordered accumulation over a transposed copy (ties are decided by rounding)
            const int ldt = ((int)o.i[2] + VW - 1) / VW * VW;
            T* wt = nullptr;
            CHK(dmalloc(&wt, (int64_t)o.i[3] * ldt * (int64_t)sizeof(T)));
            HIPCHK(ssn::launch_transpose<T>(stream, (const T*)w.d, wt, (int)o.i[2], (int)o.i[3], (int)w.ld, ldt));
            it.type = IT_MATVEC_ORDERED; it.Wm = wt; it.ld = ldt;
          }
          items.push_back(it);
          MOp g{};
          g.kind = ssn::M_ARGMAX_GATHER; g.dst = o.i[0]; g.len = o.i[3]; g.i0 = o.i[2]; g.i1 = w.ld; g.p0 = w.d; g.p1 = scratch;
          if (o.i[2] >= 65536) {
            // long similarity vector: first maxima of P slices in their own launch, the program picks among the P candidates
            const int P = (int)std::min<int64_t>(1024, (o.i[2] + 1023) / 1024);      // ~4 workgroups per CU at 10^6 rows
            T* part = nullptr;
            CHK(dmalloc(&part, P * (int64_t)(sizeof(T) + sizeof(int))));
            Item ap; ap.type = IT_ARGMAX_PART; ap.src = scratch; ap.dst = part; ap.rows = (int)o.i[2]; ap.n = P; ap.seg = gsplit;
            items.push_back(ap);
            g.p1 = part; g.src = P;
          }
          push_micro(g, o.level, true);
          break;
        }
        default: return fail(SSN_EINVAL, "unknown operator kind %d", o.kind);
      }
    }
    drain_reduces();
    auto by_order = [](const std::pair<int, ssn::BatchOp<T>>& a, const std::pair<int, ssn::BatchOp<T>>& b) { return a.first < b.first; };
    std::stable_sort(pre_sorted.begin(), pre_sorted.end(), by_order);
    std::stable_sort(post_sorted.begin(), post_sorted.end(), by_order);
    for (auto& x : pre_sorted) pre_ops.push_back(x.second);
    for (auto& x : post_sorted) post_ops.push_back(x.second);
    bool first_out = true;
    for (auto& r : core_to_post) {       // hand this timestep's results to the post stage
      if (fused) break;
      MOp op{};
      op.kind = ssn::M_ROW_OUT; op.src = r.lo; op.len = r.hi - r.lo; op.p0 = bsig; op.i0 = n_sig; op.i1 = r.lo;
      push_micro(op, -11, first_out);
      first_out = false;
    }
    bool first_probe = true;
    for (size_t p = 0; p < probes.size(); ++p) {
      if (probes[p].stage != 1) {         // sampled by the batched stages, after all their operators
        ssn::BatchOp<T> b{};
        b.bsig = bsig; b.n_sig = n_sig; b.kind = ssn::M_PROBE; b.src = probes[p].src; b.len = probes[p].width; b.p0 = d_pslots + p;
        post_ops.push_back(b);
        continue;
      }
      MOp op{};
      op.kind = ssn::M_PROBE; op.src = probes[p].src; op.len = probes[p].width; op.p0 = d_pslots + p;
      push_micro(op, -2, first_probe);
      first_probe = false;
    }
    optimise_batch(pre_ops, pre_launches);
    optimise_batch(post_ops, post_launches);
    if (!fused) {
      MOp end{};
      end.kind = ssn::M_STEP_END;
      push_micro(end, -3, false);
    }
    force_barrier = true;
    flush();
    for (auto& it : items) if (it.phase < 0) it.phase = cur_phase;      // (the tail program - probes, step counter - closes phase 1)
    if (phased && cur_phase != 1) return fail(SSN_EINVAL, "a model with exchange ranges needs operators of phase 1");
    if (best_item >= 0) {
      items[best_item].dominant = true;
      const ssn::EnsArgs<T>& a = items[best_item].ens;
      dom_units = (int64_t)a.K * a.n;
      dom_bytes = (double)dom_units * (a.din + a.dout + 5) * sizeof(T);
    }
    int n_core_ops = 0;
    for (int i = 0; i < m->n_ops; ++i) n_core_ops += m->ops[i].stage == 1;
    bool core_probe = false;
    for (auto& p : probes) core_probe = core_probe || p.stage == 1;
    core_empty = bsig && n_core_ops == 0 && !core_probe;      // (no launch per timestep then, however the plan below counts)
    round_mode = !fused && !opt.has(SSN_PLAN_NO_ROUNDS);
    if (round_mode) {
      CHK(build_rounds(programs, item_prog));
      if (core_empty) launches_per_step = 0;
      return SSN_OK;
    }
    // Sink programs: a program none of the operators up to the next program depends on (e.g. the clean-up's
    // argmax + row gather, whose result is first used after the path integrator's ensembles; the chunk reductions
    // of sparse products whose sums are first used behind the next neuron populations) joins that next program -
    // same operators, same order among dependent ones, one launch (~8 us inside the step graph) fewer each.
    if (!fused && !phased) {
      for (bool changed = true; changed;) {
        changed = false;
        analyse_dependencies(programs, item_prog);
        int pi = 0;
        for (size_t i = 0; i < items.size() && !changed; ++i) {
          if (items[i].type != IT_PROGRAM) continue;
          const int my_prog = pi++;
          if (i == 0) continue;                                  // the head starts the timestep
          size_t j = i + 1;
          bool free_to_move = true;
          for (; j < items.size() && items[j].type != IT_PROGRAM; ++j)
            for (int dep : item_deps[j]) free_to_move = free_to_move && dep != (int)i;
          if (j >= items.size() || j == i + 1 || !free_to_move) continue;
          std::vector<MOp>& dst = programs[(size_t)my_prog + 1];
          if (!dst.empty()) dst[0].barrier = 1;
          dst.insert(dst.begin(), programs[(size_t)my_prog].begin(), programs[(size_t)my_prog].end());
          programs.erase(programs.begin() + my_prog);
          items.erase(items.begin() + (long)i);
          item_prog.pop_back();
          changed = true;
        }
      }
    }
    // micro-op storage: programs in order, then a copy of the head behind the tail for the fused launch.
    // Long first level of the head program -> its own grid-wide launch (k_vecops).  The head then no longer starts the
    // timestep, so the tail / head fusion is given up: worth it from ~16 k elements on (SLAM config 3: 42 -> ~23 us).
    std::vector<MOp>& vec_ops = vecops_host;
    vec_ops.clear();
    if (!fused && !phased && !items.empty() && items.front().type == IT_PROGRAM && !programs.empty()) {
      std::vector<MOp>& head = programs[(size_t)item_prog[0]];
      size_t lv = 0;
      long long elems = 0;
      // The prefix that moves: element-wise operators up to the first barrier that are INDEPENDENT of each other.  Inside
      // a program an operator may follow one it depends on without a barrier when both map every element to the same
      // thread (push_micro); k_vecops maps elements to threads of the whole grid, so such a chain must not move as one.
      std::vector<Rng> moved, mine;                    // what the prefix so far reads and writes
      for (; lv < head.size() && (lv == 0 || !head[lv].barrier); ++lv) {
        const MOp& q = head[lv];
        if (!kind_is(q.kind, ssn::MK_VECOPS)) break;
        mine.clear();
        micro_access(mine, q, false, true);
        if (hazard(mine, moved)) break;
        moved.insert(moved.end(), mine.begin(), mine.end());
        elems += q.len;
      }
      if (elems >= 16384 && lv > 0 && lv < head.size()) {
        vec_ops.assign(head.begin(), head.begin() + (long)lv);
        head.erase(head.begin(), head.begin() + (long)lv);
        head[0].barrier = 0;
        Item vi; vi.type = IT_VECOPS; vi.n = (int)std::min<long long>(256, (elems + 2047) / 2048);
        items.insert(items.begin(), vi);
      }
    }
    int n_prog = (int)programs.size();
    mops.clear();
    prog_descs.clear();
    for (int p = 0; p < n_prog; ++p) {
      ssn::ProgDesc pd{};
      pd.op_begin = (int)mops.size(); pd.op_count = (int)programs[p].size();
      mops.insert(mops.end(), programs[p].begin(), programs[p].end());
      prog_descs.push_back(pd);
    }
    int pi = 0;
    for (auto& it : items)
      if (it.type == IT_PROGRAM) { it.op_begin = pi; it.op_count = 1; ++pi; }      // op_begin = program index
    can_fuse = !fused && !phased && items.size() >= 2 && items.front().type == IT_PROGRAM && items.back().type == IT_PROGRAM;
    if (can_fuse) {
      // the tail is the last program: a copy of the head's descriptor behind it makes [tail, head] one launch
      ssn::ProgDesc hd = prog_descs.front();
      const int hb = (int)mops.size();
      for (int j = 0; j < hd.op_count; ++j) mops.push_back(mops[(size_t)(hd.op_begin + j)]);
      mops[(size_t)hb].barrier = 1;
      hd.op_begin = hb;
      prog_descs.push_back(hd);
      tail_begin = n_prog - 1;
    }
    CHK(dupload(&d_progs, prog_descs));
    if (!vec_ops.empty()) {
      items.front().op_begin = (int)mops.size(); items.front().op_count = (int)vec_ops.size();
      mops.insert(mops.end(), vec_ops.begin(), vec_ops.end());
    }
    CHK(dupload(&d_mops, mops));
    launches_per_step = (int)items.size() - (can_fuse ? 1 : 0);
    if (fused_defer) launches_per_step = 1;
    if (fused_block) launches_per_step = 0;      // one launch per block
    if (core_empty) launches_per_step = 0;
    if (!fused) analyse_dependencies(programs, item_prog);
    if (!fused && !opt.has(SSN_PLAN_NO_ITEM_BATCH)) merge_adjacent_items();
    for (size_t i = 0; i < items.size(); ++i)        // the timestep as a launch sequence, like the round plan's
      if (!items[i].merged) launch_list.push_back(Launch{-1, (int)i, items[i].phase});
    if (opt.debug_plan) {
      int pj = 0;
      for (size_t i = 0; i < items.size(); ++i) {
        if (items[i].type != IT_PROGRAM) { fprintf(stderr, "[ssn] plan item %2zu type %d rows %d cols %d n %d\n", i, items[i].type, items[i].rows, items[i].cols, items[i].n); continue; }
        const auto& pr = programs[(size_t)item_prog[(size_t)pj++]];
        long long elems = 0; int levels = 1;
        for (size_t q = 0; q < pr.size(); ++q) { elems += pr[q].len * (pr[q].kind == ssn::M_MATVEC_INC || pr[q].kind == ssn::M_MATVEC_SET ? pr[q].i0 : 1); if (q && pr[q].barrier) ++levels; }
        fprintf(stderr, "[ssn] plan item %2zu program: %zu ops, %d levels, %lld elements:", i, pr.size(), levels, elems);
        for (auto& o : pr) fprintf(stderr, " %d/%lld", o.kind, o.len);
        fprintf(stderr, "\n");
      }
    }
    return SSN_OK;
  }


  // ---- round plan ---------------------------------------------------------------------------------------------------
  // Every micro-operator and every big operator of the timestep is a unit; a unit's round is the earliest one its data
  // hazards (RAW, WAR, WAW against every earlier unit of the sequential order) allow.  A round is launched as one k_round
  // grid (ssn_round.hpp) plus one plain launch for each operator whose kernel has no body there (ensemble arrays, the
  // ordered / factored clean-up products).
  // k_round body of an ensemble array (-1: its variant has none, it is launched on its own)
  int ens_round_kind(const ssn::EnsArgs<T>& a) const {
    // (a tapped array is launched on its own - k_ensarray's tapped twin: the bodies of the round grid do not know taps - and so
    //  is a driven one: k_ensarray_drv)
    if (a.defer || a.xrows || a.tap || a.drv_m || opt.has(SSN_PLAN_ENS_OWN_LAUNCH)) return -1;
    if (a.fast == 1 && a.din == 3 && a.dout == 4) return ssn::RK_ENS_3_4_S;
    if (a.fast == 1 && a.din == 3 && a.dout == 5) return ssn::RK_ENS_3_5_S;
    if (a.fast == 2 && a.din == 1 && a.dout == 1) {
      // many small ensembles (the product arrays of a circular convolution): a wave per ensemble instead of a workgroup
      if (a.n <= 64 && a.P == 1 && a.direct && opt.small_ens) return ssn::RK_ENS_SMALL;
      return ssn::RK_ENS_1_1_D;
    }
    return -1;
  }
  // blocks of an ensemble array's grid inside a round
  int ens_round_blocks(const ssn::EnsArgs<T>& a) const {
    return ens_round_kind(a) == ssn::RK_ENS_SMALL ? (a.K + 4 * ssn::ENS_SMALL_PER_WAVE - 1) / (4 * ssn::ENS_SMALL_PER_WAVE) : a.K * a.P;
  }

  // Cost model of the round balancer: device time a unit needs when bandwidth-bound (us at ~5 TB/s), the latency of a
  // single-workgroup unit (us), and the number of blocks of its grid (0: not splittable).
  // latency of the single-workgroup bodies as the balancer prices them (us): alone a transform takes 9.5 us and the argmax ~3; inside a
  // round that also streams they take 25 - 30 and ~13 (tools/round_stamps.py) - SSN_LAT_DFT / SSN_LAT_SOLO for A/B runs
  // (fractions of its matrix a learning rule's update is priced at: dense it reads and writes everything, in the reference's memory
  //  1.3 % of the filtered activities are nonzero - SSN_COST_PES / SSN_COST_VOJA for A/B runs)
  // tallest matrix that runs four rows per workgroup with four vectors of a row in flight per lane (one trip for 1015 columns)
  // instead of sixteen rows per workgroup with one vector of four rows in flight (four trips)
  void unit_cost(int mop, int item, double* us, double* lat, int* blocks) const {
    *us = 0.0; *lat = 0.0; *blocks = 0;
    const double per_us = 5.0e6;      // bytes per microsecond
    if (mop >= 0) {
      const MOp& op = mops[(size_t)mop];
      if (op.kind == ssn::M_GATE || op.kind == ssn::M_ARGMAX_GATHER) *lat = opt.lat_solo;
      else *us = (double)op.len * 3.0 * sizeof(T) / per_us;
      return;
    }
    const Item& it = items[(size_t)item];
    switch (it.type) {
      case IT_ENS:
        *us = (double)it.ens.K * it.ens.n_pad * (it.ens.din + 4.5) * sizeof(T) / per_us;
        if (ens_round_kind(it.ens) >= 0) *blocks = ens_round_blocks(it.ens);
        break;
      case IT_MATVEC:
        *us = (double)it.rows * it.ld * sizeof(T) / per_us;
        if ((size_t)it.cols * sizeof(T) <= 48 * 1024) *blocks = it.rows <= opt.matvec_r1_max ? (it.rows + 3) / 4 : (it.rows + 15) / 16;
        break;
      case IT_PES: *us = opt.cost_pes * it.rows * it.ld * sizeof(T) / per_us; *blocks = ((it.cols + 1023) / 1024) * ((it.rows + ssn::PES_ROWS - 1) / ssn::PES_ROWS); break;
      case IT_VOJA: *us = opt.cost_voja * it.rows * it.ld * sizeof(T) / per_us; break;
      case IT_SPMV: *us = 0.1 * (double)it.cols * it.ld * sizeof(T) / per_us; break;
      case IT_NEURONS: *us = (double)it.n * 5.0 * sizeof(T) / per_us; break;
      case IT_MATVEC_NEURONS: *us = (double)it.rows * it.ld * sizeof(T) / per_us; *blocks = (it.rows + 15) / 16; break;
      case IT_DFT: *lat = opt.lat_dft; break;
      default: *us = 1.0; break;
    }
  }

  // Round balancer of the pipelined plan.  The earliest-round assignment stacks the bandwidth-bound operators of a
  // timestep in a few rounds and leaves others with one latency-bound workgroup (a DFT) and an idle chip.  Every block of
  // a grid is independent, so a heavy operator may run in pieces: any round from its own up to the last one before its
  // first conflicting successor is valid for any of its blocks (successors were placed later than that, predecessors
  // earlier; pieces only ever move later, which keeps every other window valid).  Heavy instances are poured, a
  // thirty-second at a time, into the round of their window where the quantum costs least (free under a latency-bound
  // round's critical workgroup; otherwise the least loaded).
  template <typename Inst, typename H, typename C>
  void balance_rounds(std::vector<Inst>& all, int nr, size_t per, H conflict, C cost) {
    const size_t N = all.size();
    std::vector<double> load((size_t)nr, 0.0), lat((size_t)nr, 0.0);
    std::vector<double> us(N, 0.0);
    std::vector<int> blocks(N, 0);
    std::map<int, double> serial;
    for (size_t i = 0; i < N; ++i) {
      double l = 0.0;
      cost(all[i].unit, &us[i], &l, &blocks[i]);
      load[(size_t)all[i].round] += us[i];
      if (all[i].solo && all[i].chain >= 0) { serial[all[i].chain] += std::max(l, 1.0 + us[i]); l = serial[all[i].chain]; }      // a serial chain: one block, members back to back
      lat[(size_t)all[i].round] = std::max(lat[(size_t)all[i].round], l);
    }
    std::vector<Inst> extra;
    for (size_t i = 0; i < N; ++i) {
      if (us[i] < 4.0 || blocks[i] < 64) continue;            // heavy: >= ~20 MB
      const int r0 = all[i].round;
      int r1 = nr - 1;
      const size_t stop = std::min(N, ((size_t)all[i].sub + 2) * per);
      for (size_t j = i + 1; j < stop; ++j)
        if (all[j].round - 1 < r1 && conflict(all[i].unit, all[j].unit)) r1 = all[j].round - 1;
      if (r1 <= r0) continue;
      load[(size_t)r0] -= us[i];
      const int Q = 32;
      const double q = us[i] / Q;
      std::vector<int> share((size_t)(r1 - r0 + 1), 0);
      for (int k = 0; k < Q; ++k) {
        int best = r0;
        double best_cost = 1e30, best_load = 1e30;
        for (int r = r0; r <= r1; ++r) {
          const double before = std::max(load[(size_t)r], lat[(size_t)r]), after = std::max(load[(size_t)r] + q, lat[(size_t)r]);
          const double c = after - before;
          if (c < best_cost - 1e-9 || (c < best_cost + 1e-9 && load[(size_t)r] < best_load)) { best = r; best_cost = c; best_load = load[(size_t)r]; }
        }
        share[(size_t)(best - r0)] += 1;
        load[(size_t)best] += q;
      }
      int lo = 0, used = 0;
      bool first = true;
      for (int r = r0; r <= r1; ++r) {
        const int sh = share[(size_t)(r - r0)];
        if (!sh) continue;
        used += sh;
        const int hi = used == Q ? blocks[i] : (int)((long long)blocks[i] * used / Q);
        if (hi <= lo) continue;
        if (first) { all[i].round = r; all[i].lo = lo; all[i].cnt = hi - lo; first = false; }
        else { Inst p = all[i]; p.round = r; p.lo = lo; p.cnt = hi - lo; extra.push_back(p); }
        lo = hi;
      }
    }
    all.insert(all.end(), extra.begin(), extra.end());
    if (opt.debug_plan) {          // what the balancer believes the rounds cost (us): bandwidth-bound load | longest single-workgroup body
      fprintf(stderr, "[ssn] balanced rounds (load | latency, us):");
      double total = 0.0;
      for (int r = 0; r < nr; ++r) { fprintf(stderr, " %.0f|%.0f", load[(size_t)r], lat[(size_t)r]); total += std::max(load[(size_t)r], lat[(size_t)r]); }
      fprintf(stderr, "\n[ssn] sum of max(load, latency) over %d rounds: %.0f us\n", nr, total);
    }
  }

  // ---- build_rounds: its working state and its steps, in the order the driver at the end calls them ----------------------
  struct Unit { int mop = -1; int item = -1; int phase = 0; bool writes = false; std::vector<Rng> acc; };
  // One instance of a unit: (unit, timestep offset inside the launch sequence, round).
  struct Inst { int unit; int sub; int round; int lo = 0; int cnt = -1; int chain = -1; bool solo = false; };      // blocks [lo, lo + cnt) of the unit's grid (cnt < 0: all); solo: member of a serial chain
  struct Fix { size_t rl; int entry; int what; size_t off; };     // what: 0 arena, 1 glue map, 2 micro-operator, 3 chain table
  typedef std::vector<std::vector<Rng>> AccLists;      // access list per unit
  typedef std::vector<std::vector<int>> Chains;        // members (indices into the instance list) per chain
  struct SeqOp { int item; int prog; int op; std::vector<Rng> acc; };      // an operator in program order (prog / op: -1 for a big operator)
  struct RoundBuild {
    std::vector<Unit> units;
    std::vector<ssn::GlueBlock> glue_map;      // block -> (operator, chunk) of the glue entries
    std::vector<unsigned char> arena;          // body arguments of the big operators
    std::vector<long long> unit_arg;           // arena offset of a big operator's body arguments (shared by its instances)
    std::vector<Fix> fixes;                    // device pointers the round entries get once the tables are uploaded
    std::vector<int> chain_tab;
    size_t put(const void* src, size_t bytes) { const size_t off = (arena.size() + 15) / 16 * 16; arena.resize(off + bytes); memcpy(arena.data() + off, src, bytes); return off; }
  };

  // accesses of every operator in program order (the rewrite passes below and the cuts scan this list)
  std::vector<SeqOp> program_order(const std::vector<std::vector<MOp>>& programs, const std::vector<int>& item_prog) const {
    std::vector<SeqOp> seq;
    int pj = 0;
    for (size_t i = 0; i < items.size(); ++i) {
      if (items[i].type == IT_PROGRAM) {
        const int pr = item_prog[(size_t)pj++];
        for (size_t q = 0; q < programs[(size_t)pr].size(); ++q) { seq.push_back(SeqOp{(int)i, pr, (int)q, {}}); micro_access(seq.back().acc, programs[(size_t)pr][q], false); }
      } else {
        seq.push_back(SeqOp{(int)i, -1, -1, {}});
        item_access(seq.back().acc, items[i]);
      }
    }
    return seq;
  }

  // Round 4: the critical recurrence of a SLAM timestep - memory spikes -> sparse decode -> PES (may not touch W before the
  // decode has read it) -> filter of the activities PES reads (may not run before PES) -> next timestep's spikes (may not
  // overwrite what that filter reads) - is four rounds of WAR hazards.  The filter update folded into the PES body (the
  // workgroup that has read row r's factor advances it) takes one of them out.  Round 2 measured this fold slower because the
  // oscillators' own four-round recurrence kept the period at four.  SSN_PES_FOLD=0: off.
  // The filter update follows the rule in program order (reads before updates); nothing between the two may touch the filter's state
  // or write its input, or the update could not move up to the rule.
  void fold_pes_filters(std::vector<std::vector<MOp>>& programs, const std::vector<int>& item_prog) {
    if (!((!phased || opt.phased_pes_fold) && opt.pes_fold)) return;
    for (size_t i = 0; i < items.size(); ++i) {
      Item& pe = items[i];
      if (pe.type != IT_PES || pe.cols > 1024 || !(pe.aux0 >= sig && pe.aux0 < sig + n_sig)) continue;
      const long long f0 = pe.aux0 - sig;
      const std::vector<SeqOp> seq = program_order(programs, item_prog);
      size_t at = 0;
      while (seq[at].item != (int)i) ++at;
      for (size_t e = at + 1; e < seq.size(); ++e) {
        if (seq[e].prog < 0) continue;
        std::vector<MOp>& pr = programs[(size_t)seq[e].prog];
        const MOp& lp = pr[(size_t)seq[e].op];
        if (!(lp.kind == ssn::M_LOWPASS && lp.dst == f0 && lp.len == pe.rows)) continue;
        bool clear = true;
        for (size_t v = at + 1; v < e && clear; ++v) clear = !hazard(seq[v].acc, seq[e].acc);
        if (clear) {
          pe.lp_dst = sig + lp.dst; pe.lp_src = sig + lp.src; pe.lp_a = lp.a; pe.lp_b = lp.b;
          pr.erase(pr.begin() + seq[e].op);
        }
        break;
      }
    }
  }

  // Round 4: the neuron update of a dense population in the epilogue of its encoder product.  A population hop is four
  // dependent rounds - product (J += W x) -> neurons -> sparse decode over the spike list -> reduction (+ filter) - and a
  // neuron-sharded timestep adds the exchange and the filter behind it: six rounds between two exchanges.  Where the product is
  // the last writer of the current vector J before the neurons, nothing else ever reads J, and nothing between the two touches
  // the product's operands, the workgroup that owns 16 rows steps their 16 neurons itself (matvec_neurons_body).  The fused
  // operator takes the neurons' place in program order (whatever reads the previous timestep's spikes between the two still
  // comes first).  SSN_FUSE_NEURONS=0: off.
  int fuse_product_neurons(const std::vector<std::vector<MOp>>& programs, const std::vector<int>& item_prog) {
    if (!opt.fuse_neurons) return SSN_OK;
    const std::vector<SeqOp> seq = program_order(programs, item_prog);
    for (size_t jn = 0; jn < items.size(); ++jn) {
      Item& N = items[jn];
      if (N.type != IT_NEURONS || !(N.src >= sig && N.src < sig + n_sig)) continue;
      const int64_t j0 = N.src - sig, j1 = j0 + N.n;
      int jm = -1;
      for (size_t j = 0; j < jn; ++j)
        if (items[j].type == IT_MATVEC && items[j].dst == N.src && items[j].rows == N.n) jm = (int)j;
      if (jm < 0) continue;
      const Item& M = items[(size_t)jm];
      // (smaller populations keep the four-rows-per-workgroup product, which fills more of the chip; SSN_FUSE_MIN_ROWS for tests)
      if ((size_t)M.cols * sizeof(T) > 48 * 1024 || M.rows < opt.fuse_min_rows || M.phase != N.phase) continue;
      std::vector<Rng> accM;
      item_access(accM, M);
      bool ok = true;
      for (const auto& e : seq) {
        if (e.item == jm || e.item == (int)jn) continue;
        for (const Rng& r : e.acc) {
          if (r.space != (const void*)sig || r.lo >= j1 || j0 >= r.hi) continue;
          if (!r.w) ok = false;                                        // another reader of J
          else if (e.item > jm && e.item < (int)jn) ok = false;      // another writer between the product and the neurons
          else if (e.item > (int)jn) ok = false;                      // (a writer behind the neurons: not the pattern)
        }
        if (e.item > jm && e.item < (int)jn && hazard(e.acc, accM)) ok = false;      // the product's operands change on the way
        if (!ok) break;
      }
      if (!ok) continue;
      if (N.list) {                        // spike list in 16-neuron segments: counts per small segment, the spans of the products stay
        int* cnt = nullptr;
        const int n_small = (N.n + 15) / 16;
        CHK(dzeros(&cnt, (int64_t)n_small + 16));
        for (Item& sp : items) if (sp.type == IT_SPMV && sp.list == N.list) { sp.count = cnt; sp.seg_len = 16; }
        N.count = cnt;
      }
      N.type = IT_MATVEC_NEURONS;
      N.Wm = M.Wm; N.aux0 = M.src; N.rows = M.rows; N.cols = M.cols; N.ld = M.ld; N.set = M.set;
      items[(size_t)jm].type = IT_NONE;
      n_fused_populations += 1;
      if (opt.debug_plan) fprintf(stderr, "[ssn] encoder product %d x %d and the update of its %d neurons fused (items %d, %zu)\n", N.rows, N.cols, N.n, jm, jn);
    }
    return SSN_OK;
  }

  // Element-wise micro-operators are cut at every range endpoint of the other operators.  The builder merges
  // neighbouring resets / hand-offs into one long operator (one fill over all accumulators of a network); as a unit
  // it would inherit the hazards of every signal it spans - the reset of an accumulator that is read in the last
  // round of step s would hold back the whole head of step s + 1.
  std::vector<int64_t> range_cuts(const std::vector<std::vector<MOp>>& programs, const std::vector<int>& item_prog) const {
    std::vector<int64_t> cuts;
    for (const SeqOp& e : program_order(programs, item_prog))
      for (const Rng& r : e.acc) if (r.space == (const void*)sig) { cuts.push_back(r.lo); cuts.push_back(r.hi); }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    return cuts;
  }
  int split_micro(const MOp& op, const std::vector<int64_t>& cuts, std::vector<MOp>& out) {
    if (!kind_is(op.kind, ssn::MK_CUT) || op.len <= 1 || opt.has(SSN_PLAN_NO_CUTS)) { out.push_back(op); return SSN_OK; }
    std::vector<Rng> operands;                        // (their origins in signal space: every one is op.len long)
    micro_access(operands, op);
    const std::vector<ssn::LinTerm<T>>* terms = nullptr;
    if (op.kind == ssn::M_LINCOMB) { auto f = lin_terms.find(op.p0); if (f != lin_terms.end()) terms = &f->second; }
    std::vector<int64_t> offs{0, op.len};
    for (const Rng& r : operands) {
      const int64_t b = r.lo;
      auto lo = std::upper_bound(cuts.begin(), cuts.end(), b), hi = std::lower_bound(cuts.begin(), cuts.end(), b + op.len);
      for (auto it = lo; it < hi; ++it) offs.push_back(*it - b);
    }
    std::sort(offs.begin(), offs.end());
    offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
    if (offs.size() > 64) { out.push_back(op); return SSN_OK; }       // (pathological fragmentation: keep the operator whole)
    for (size_t q = 0; q + 1 < offs.size(); ++q) {
      const int64_t o = offs[q];
      MOp pc = op;
      pc.len = offs[q + 1] - o;
      pc.dst = op.dst + o;
      if (op.kind == ssn::M_AXPY_INC || op.kind == ssn::M_AXPY_SET || op.kind == ssn::M_LOWPASS || op.kind == ssn::M_ROW_OUT) pc.src = op.src + o;
      if (op.kind == ssn::M_ROW_IN || op.kind == ssn::M_ROW_OUT) pc.i1 = op.i1 + o;
      if (terms && o != 0) {
        std::vector<ssn::LinTerm<T>> tt = *terms;
        for (auto& t : tt) t.src += o;
        ssn::LinTerm<T>* d_terms = nullptr;
        CHK(dupload(&d_terms, tt));
        lin_terms[(const void*)d_terms] = tt;
        pc.p0 = d_terms;
      }
      out.push_back(pc);
    }
    return SSN_OK;
  }

  // every micro-operator (cut into pieces) and every big operator of the timestep as a unit, in program order
  int make_units(RoundBuild& b, const std::vector<std::vector<MOp>>& programs, const std::vector<int>& item_prog) {
    const std::vector<int64_t> cuts = range_cuts(programs, item_prog);
    mops.clear();
    int prog_i = 0;
    for (size_t i = 0; i < items.size(); ++i) {
      const Item& it = items[i];
      if (it.type == IT_PROGRAM) {
        std::vector<MOp> pieces;
        for (const MOp& op0 : programs[(size_t)item_prog[(size_t)prog_i]]) CHK(split_micro(op0, cuts, pieces));
        for (const MOp& op0 : pieces) {
          MOp op = op0;
          op.barrier = 0;
          Unit u; u.mop = (int)mops.size(); u.phase = std::max(0, it.phase);
          micro_access(u.acc, op, true);
          mops.push_back(op);
          b.units.push_back(std::move(u));
        }
        ++prog_i;
      } else if (it.type != IT_NONE) {
        Unit u; u.item = (int)i; u.phase = std::max(0, it.phase);
        item_access(u.acc, it);
        b.units.push_back(std::move(u));
      }
    }
    for (Unit& u : b.units) for (const Rng& r : u.acc) u.writes = u.writes || r.w;
    b.unit_arg.assign(b.units.size(), -1);
    CHK(dupload(&d_mops, mops));
    return SSN_OK;
  }

  // Chains: an element-wise micro-operator whose only hazards inside a round are with other element-wise micro-operators
  // on the SAME elements (equal ranges: a filter update behind the reduction it filters, the next step's input hand-off
  // behind that update) joins their round - one block then runs the chain's operators back to back on 256 elements, the
  // same thread on the same index in program order, with no barrier and no launch between them.
  bool chainable(const Unit& u) const {
    return u.mop >= 0 && !opt.has(SSN_PLAN_NO_CHAINS) && kind_is(mops[(size_t)u.mop].kind, ssn::MK_CHAIN);
  }
  // Serial chains (round 4, second half).  The long loop of a SLAM timestep - clean-up -> binding -> memory -> unbinding -> gate ->
  // oscillator input, one synapse delay per hop - is partly made of operators that ONE workgroup executes: glue over 1 - 2
  // thousand elements, the gate, the argmax + gather, the transforms of the circular convolutions.  A single-workgroup unit
  // whose only predecessors in the round before its own are members of one such chain (or one such unit) joins it instead of
  // opening a round: the chain's block (RK_SOLO, solo_body) runs its members in program order with a workgroup barrier
  // between them - results pass through global memory inside one workgroup, workgroup-scope visibility is all that needs.
  // Measured at SLAM config 3 (profiles/round4_serial_chains.txt): a member costs ~2 us (one trip for its data, one for its
  // store to land before the barrier; ~4 us before the members' descriptors were staged in LDS), a transform ~9.5 us.
  //   * glue / gate / argmax members only (default): 102.7 vs 104.7 us per timestep, any cap between 8 and 24 us;
  //   * with the transforms as members (SSN_SOLO_DFT=1) the plan drops from 3.78 to 3.0 - 3.3 rounds per timestep and gets
  //     SLOWER - 110.8 us at a cap of 12 us, 114.8 at 16, 129 at 22, 139 at 26: a round now lasts as long as its longest
  //     chain (transform + members: 20 - 45 us) and the bandwidth-bound work does not fill the time under it;
  //   * neuron-sharded plans: nothing for the per-timestep phases (157.8 vs 155.3 us, ten launches either way); with the
  //     plan pipelined over the exchange 123.0 vs 125.6 us at world 1 (72 vs 76 launches per 16 timesteps) - on there too
  //     (SSN_PHASED_SOLO=0: off for sharded plans only).
  // SSN_SOLO_CHAINS=0: off; SSN_SOLO_CAP_US: longest serial chain in estimated microseconds (default 16); SSN_SOLO_MAX_LEN:
  // longest glue operator a single workgroup takes (default 2048 elements).
  // LDS bytes of a transform as a round body
  static size_t dft_lds(const Item& it) {
    return ssn::fft::lds_bytes(it.dft.M > 0 ? it.dft.M : it.dft.N, it.dft.inplace != 0, it.dft.N1, it.dft.radix, it.dft.nr);
  }
  double solo_lat(const Unit& u) const {        // estimated serial time of the unit on one workgroup; < 0: not eligible
    const bool solo_on = !(phased && !opt.phased_solo) && !opt.has(SSN_PLAN_NO_CHAINS) && opt.solo_chains;
    if (!solo_on) return -1.0;
    if (u.mop >= 0) {
      const MOp& op = mops[(size_t)u.mop];
      // (measured on the chains of SLAM config 3: ~2 us per glue member - one trip for its data, one for the store to land
      //  before the barrier - with its descriptor already in LDS; a transform ~9.5 us)
      if (kind_is(op.kind, ssn::MK_SAME_THREAD))
        return op.len <= opt.solo_max_len ? 1.7 + 0.5 * (double)((op.len + ssn::GLUE_CHUNK - 1) / ssn::GLUE_CHUNK) : -1.0;
      switch (op.kind) {
        case ssn::M_GATE: case ssn::M_ARGMAX_GATHER: return 3.5;
        case ssn::M_LINCOMB:
          return op.len <= opt.solo_max_len ? 1.7 + (0.5 + 0.1 * (double)op.i0) * (double)((op.len + ssn::GLUE_CHUNK - 1) / ssn::GLUE_CHUNK) : -1.0;
        case ssn::M_REDUCE_SET: case ssn::M_REDUCE_INC:
          return op.len <= opt.solo_max_len ? 1.7 + (double)((op.len + ssn::GLUE_ROWS - 1) / ssn::GLUE_ROWS) * (0.6 + 0.15 * (double)((op.i0 + 7) / 8)) : -1.0;
        default: return -1.0;
      }
    }
    if (u.item < 0) return -1.0;            // (the exchange of a sharded cycle plan)
    const Item& it = items[(size_t)u.item];
    if (opt.solo_dft && it.type == IT_DFT && it.dft.N1 == 0 && sizeof(T) == 4 && dft_lds(it) <= 60 * 1024) return 9.5;
    return -1.0;
  }
  // 0: no hazard, 1: hazards only on identical signal ranges (element-aligned), 2: any other hazard
  int conflict_kind(const std::vector<Rng>& x, const std::vector<Rng>& y) const {
    int kind = 0;
    for (const Rng& p : x)
      for (const Rng& q : y)
        if (p.space == q.space && p.lo < q.hi && q.lo < p.hi && (p.w || q.w)) {
          if (p.space == (const void*)sig && p.lo == q.lo && p.hi == q.hi) kind = std::max(kind, 1);
          else return 2;
        }
    return kind;
  }
  // round of a new instance given the instances it may conflict with; joins a chain where it can
  int place(const RoundBuild& b, std::vector<Inst>& placed, size_t from, int unit, const AccLists& accs, int base_round, Chains& chains) const {
    const Unit& uu = b.units[(size_t)unit];
    const bool can = chainable(uu);
    const long long len = can ? (long long)mops[(size_t)uu.mop].len : 0;
    int r_hard = base_round, r_soft = -1;
    std::vector<size_t> soft, hard;
    for (size_t v = from; v < placed.size(); ++v) {
      if (placed[v].round < r_hard - 1 && placed[v].round < r_soft) continue;      // can neither raise a bound nor be a chain partner
      const Unit& vv = b.units[(size_t)placed[v].unit];
      const bool both = can && chainable(vv) && (long long)mops[(size_t)vv.mop].len == len;
      const int k = both ? conflict_kind(accs[(size_t)unit], accs[(size_t)placed[v].unit])
                         : (hazard(accs[(size_t)unit], accs[(size_t)placed[v].unit]) ? 2 : 0);
      // (the exchange of a sharded cycle plan is no kernel: it happens in front of its round's launch, so what waits for it may
      //  run in that very round)
      if (k == 2) { r_hard = std::max(r_hard, placed[v].round + ((vv.mop < 0 && vv.item < 0) ? 0 : 1)); hard.push_back(v); }
      else if (k == 1) { r_soft = std::max(r_soft, placed[v].round); soft.push_back(v); }
    }
    // serial chain: every hard predecessor in round r_hard - 1 is a single-workgroup unit of ONE chain (or one such unit alone)
    const double my_lat = solo_lat(uu);
    if (my_lat >= 0.0 && r_hard - 1 >= base_round && r_hard - 1 > r_soft) {
      int chain = -2;               // -2: none seen, -3: not joinable, -1: one unchained instance (lone), >= 0: a chain
      size_t lone = 0;
      for (size_t v : hard) {
        if (placed[v].round != r_hard - 1) continue;
        if (solo_lat(b.units[(size_t)placed[v].unit]) < 0.0 || placed[v].cnt >= 0) { chain = -3; break; }
        if (placed[v].chain >= 0) {
          if (chain == -2) chain = placed[v].chain;
          else if (chain != placed[v].chain) { chain = -3; break; }
        } else {
          if (chain == -2) { chain = -1; lone = v; }
          else { chain = -3; break; }
        }
      }
      if (chain >= 0 || chain == -1) {
        double total = my_lat;
        bool ok = true;
        int transforms = uu.mop < 0 ? 1 : 0;        // (at most one per chain: solo_body runs it outside its member loops)
        if (chain >= 0 && chains[(size_t)chain].size() + 1 > (size_t)ssn::SOLO_MAX_MEMBERS) ok = false;
        if (chain == -1) { total += solo_lat(b.units[(size_t)placed[lone].unit]); transforms += b.units[(size_t)placed[lone].unit].mop < 0 ? 1 : 0; }
        else
          for (int mi : chains[(size_t)chain]) {
            const double l = solo_lat(b.units[(size_t)placed[(size_t)mi].unit]);
            if (l < 0.0 || placed[(size_t)mi].round != r_hard - 1) { ok = false; break; }
            total += l;
            transforms += b.units[(size_t)placed[(size_t)mi].unit].mop < 0 ? 1 : 0;
          }
        if (ok && transforms <= 1 && total <= opt.solo_cap_us) {
          if (chain == -1) { chain = (int)chains.size(); placed[lone].chain = chain; chains.push_back({(int)lone}); }
          for (int mi : chains[(size_t)chain]) placed[(size_t)mi].solo = true;
          Inst in{unit, 0, r_hard - 1, 0, -1, chain, true};
          chains[(size_t)chain].push_back((int)placed.size());
          placed.push_back(in);
          return in.round;
        }
      }
    }
    Inst in{unit, 0, std::max(r_hard, r_soft), 0, -1, -1};
    if (r_soft >= 0 && r_soft >= r_hard) {
      int chain = -2;
      for (size_t v : soft) {
        if (placed[v].round != r_soft) continue;
        if (placed[v].chain < 0) { placed[v].chain = (int)chains.size(); chains.push_back({(int)v}); }
        if (chain == -2) chain = placed[v].chain;
        else if (chain != placed[v].chain) chain = -3;
      }
      if (chain >= 0 && placed[(size_t)chains[(size_t)chain][0]].solo && chains[(size_t)chain].size() + 1 > (size_t)ssn::SOLO_MAX_MEMBERS) chain = -3;
      if (chain >= 0) { in.chain = chain; in.solo = placed[(size_t)chains[(size_t)chain][0]].solo; chains[(size_t)chain].push_back((int)placed.size()); }
      else in.round = r_soft + 1;            // element-aligned with members of two chains: a round of its own
    }
    placed.push_back(in);
    return in.round;
  }

  // k_round body of a big operator: kind, grid and LDS bytes; its arguments go to the arena once (ao: their offset, shared by the
  // operator's instances).  kind < 0: the operator has no body there and is launched on its own.
  struct RoundBody { int kind = -1; int gx = 1, gy = 1; size_t lds = 0; };
  RoundBody round_body(RoundBuild& b, const Item& it, long long& ao) const {
    const size_t xb = (size_t)it.cols * sizeof(T);
    switch (it.type) {
      case IT_MATVEC:
        if (xb <= 48 * 1024) {
          const bool r1 = it.rows <= opt.matvec_r1_max;
          if (r1) {
            ssn::MatvecArgs<T> a{it.Wm, it.src, it.dst, it.rows, it.cols, it.ld, it.set};
            if (ao < 0) ao = (long long)b.put(&a, sizeof a);
          } else {                 // (the 16-rows-per-workgroup body is matvec_neurons_body's: no population behind this product)
            ssn::MatvecNeuronsArgs<T> a{};
            a.mv = ssn::MatvecArgs<T>{it.Wm, it.src, it.dst, it.rows, it.cols, it.ld, it.set};
            if (ao < 0) ao = (long long)b.put(&a, sizeof a);
          }
          return RoundBody{r1 ? ssn::RK_MATVEC_R1 : ssn::RK_MATVEC_R4, r1 ? (it.rows + 3) / 4 : (it.rows + 15) / 16, 1, (xb + 15) / 16 * 16 + 64};
        }
        break;
      case IT_ENS: {
        const ssn::EnsArgs<T>& a = it.ens;
        const int kind = ens_round_kind(a);
        if (kind >= 0) {
          if (ao < 0) ao = (long long)b.put(&a, sizeof a);
          return RoundBody{kind, ens_round_blocks(a), 1, 512};
        }
        break;
      }
      case IT_SPMV: {
        ssn::SpmvArgs<T> a{it.Wm, it.ld, it.src, it.cols, it.rows, it.dst, it.ld, it.n, it.list, it.count, it.seg, it.seg_len};
        const size_t lds = 272 * sizeof(int) + (it.list ? 0 : (size_t)it.cols * sizeof(int));
        if (lds <= 60 * 1024) {
          if (ao < 0) ao = (long long)b.put(&a, sizeof a);
          return RoundBody{ssn::RK_SPMV, (it.rows + 255) / 256, it.n, lds};
        }
        break;
      }
      case IT_NEURONS: {
        ssn::NeuronsArgs<T> a{it.np, it.src, it.dst, it.V, it.R, it.n, it.scalar, it.list, it.count};
        if (ao < 0) ao = (long long)b.put(&a, sizeof a);
        return RoundBody{ssn::RK_NEURONS, (it.n + 255) / 256, 1, 64};
      }
      case IT_MATVEC_NEURONS: {
        ssn::MatvecNeuronsArgs<T> a{ssn::MatvecArgs<T>{it.Wm, it.aux0, nullptr, it.rows, it.cols, it.ld, it.set},
                                    ssn::NeuronsArgs<T>{it.np, it.src, it.dst, it.V, it.R, it.n, it.scalar, it.list, it.count}};
        if (ao < 0) ao = (long long)b.put(&a, sizeof a);
        return RoundBody{ssn::RK_MATVEC_NEURONS, (it.rows + 15) / 16, 1, (xb + 15) / 16 * 16 + 64};
      }
      case IT_DFT: {
        const size_t lds = dft_lds(it);
        if (lds <= 64 * 1024 && it.dft.N1 == 0) {      // (the four-step engine is launched on its own: see dft_body<ROUND>)
          if (ao < 0) ao = (long long)b.put(&it.dft, sizeof it.dft);
          return RoundBody{ssn::RK_DFT, 1, 1, lds};
        }
        break;
      }
      case IT_GRID_LHS: {
        ssn::GridLhsArgs<T> a{it.src, it.aux0, it.ld, it.dst, it.cols, it.rows, it.cols / 2};
        if (ao < 0) ao = (long long)b.put(&a, sizeof a);
        return RoundBody{ssn::RK_GRID_LHS, (it.rows * (it.cols / 2) + 255) / 256, 1, 64};
      }
      case IT_GRID_DOT: {
        ssn::GridDotArgs<T> a{it.src, it.cols, it.Wm, it.ld, it.dst, it.n, it.cols, it.rows};
        if (ao < 0) ao = (long long)b.put(&a, sizeof a);
        return RoundBody{ssn::RK_GRID_DOT, (it.n + 15) / 16, it.rows, xb};
      }
      case IT_PES: {
        ssn::PesArgs<T> a{it.Wm, it.aux0, it.aux1, it.rows, it.cols, it.ld, it.scalar, it.lp_dst, it.lp_src, it.lp_a, it.lp_b};
        if (ao < 0) ao = (long long)b.put(&a, sizeof a);
        return RoundBody{ssn::RK_PES, (it.cols + 1023) / 1024, (it.rows + ssn::PES_ROWS - 1) / ssn::PES_ROWS, 64};
      }
      case IT_VOJA: {
        ssn::VojaArgs<T> a{it.Wm, it.src, it.aux0, it.aux1, it.aux2, it.rows, it.cols, it.ld, it.scalar};
        if (ao < 0) ao = (long long)b.put(&a, sizeof a);
        return RoundBody{ssn::RK_VOJA, (it.rows + 4 * ssn::VOJA_ROWS_PER_WAVE - 1) / (4 * ssn::VOJA_ROWS_PER_WAVE), 1, 64};
      }
      default: break;
    }
    return RoundBody{};
  }

  // Launch sequence of a set of instances grouped by round (instances of one round are mutually independent).
  void emit(RoundBuild& b, const std::vector<Inst>& insts, int n_rounds, std::vector<Launch>& out, const Chains& chains) {
    std::vector<std::vector<const Inst*>> by_round((size_t)n_rounds);
    for (const Inst& in : insts) by_round[(size_t)in.round].push_back(&in);
    auto in_chain = [&](const Inst* in) { return in->chain >= 0 && chains[(size_t)in->chain].size() >= 2; };
    for (int r = 0; r < n_rounds; ++r) {
      RoundLaunch rl;
      rl.round = r;
      rl.args = ssn::RoundArgs<T>{};
      rl.args.mops = d_mops; rl.args.sig = sig; rl.args.ctx = d_ctx;
      int phase = 0;
      std::vector<Launch> plain;
      auto close = [&]() {
        if (rl.args.n == 0) return;
        // interleaved dispatch of the big grids behind the latency-bound head (RoundArgs::stride)
        rl.args.head = 0; rl.args.stride = 0;
        int head = 0;
        for (int q = 0; q < rl.args.n; ++q) {
          const int k = rl.args.e[q].kind;
          if (k == ssn::RK_DFT || k == ssn::RK_SOLO || k == ssn::RK_GATE || k == ssn::RK_ARGMAX || k == ssn::RK_GLUE) head = rl.args.e[q].first + rl.args.e[q].cnt;
          else break;
        }
        rl.args.prio = (opt.head_prio && head < rl.n_blocks) ? head : 0;      // (blocks [0, prio) raise their waves' issue priority)
        if (opt.round_interleave) {
          const long long m = (long long)rl.n_blocks - head;
          if (m >= 64) {
            long long st = (long long)(0.6180339887 * (double)m);
            auto gcd = [](long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; };
            while (st > 1 && gcd(st, m) != 1) --st;
            if (st > 1) { rl.args.head = head; rl.args.stride = (unsigned int)st; }
          }
        }
        Launch l; l.rl = (int)round_launches.size(); l.phase = phase;
        rl.args.pad = l.rl;                    // (launch id: read by the diagnostic stamps of k_round, SSN_ROUND_STAMPS)
        round_launches.push_back(rl);
        out.push_back(l);
        rl.args.n = 0; rl.n_blocks = 0; rl.lds = 0;
      };
      int part_lo = 0, part_cnt = -1;      // block range of the instance being emitted (set per instance below)
      // The grid's blocks are dispatched in order: single-workgroup bodies whose latency bounds the round (a DFT: ~9 us)
      // go first so that they run beside the bandwidth-bound blocks instead of behind them; then the small glue; then
      // the big grids, longest first.
      struct Pending { int kind, gx, gy, what, lo, cnt; size_t lds, off; };
      std::vector<Pending> pending;
      auto entry = [&](int kind, int gx, int gy, size_t lds, int what, size_t off) {
        Pending q{kind, std::max(1, gx), std::max(1, gy), what, 0, 0, lds, off};
        q.lo = part_cnt < 0 ? 0 : part_lo;
        q.cnt = part_cnt < 0 ? q.gx * q.gy : std::min(part_cnt, q.gx * q.gy - q.lo);
        pending.push_back(q);
      };
      auto flush_entries = [&]() {
        auto prio = [](const Pending& q) { return (q.kind == ssn::RK_DFT || q.kind == ssn::RK_SOLO) ? 0 : (q.kind == ssn::RK_GATE || q.kind == ssn::RK_ARGMAX) ? 1 : q.kind == ssn::RK_GLUE ? 2 : 3; };
        std::stable_sort(pending.begin(), pending.end(), [&](const Pending& a, const Pending& b) {
          if (prio(a) != prio(b)) return prio(a) < prio(b);
          return prio(a) == 3 && a.cnt > b.cnt;
        });
        for (const Pending& q : pending) {
          if (rl.args.n == ssn::MAX_ROUND_ENTRIES) close();
          ssn::RoundEntry& e = rl.args.e[rl.args.n];
          e.kind = q.kind; e.first = rl.n_blocks; e.gx = q.gx; e.gy = q.gy; e.args = nullptr; e.lo = q.lo; e.cnt = q.cnt;
          b.fixes.push_back(Fix{round_launches.size(), rl.args.n, q.what, q.off});
          rl.n_blocks += e.cnt;
          rl.lds = std::max(rl.lds, q.lds);
          rl.args.n += 1;
        }
        pending.clear();
      };
      // the exchange of a neuron-sharded cycle plan (a unit without operator): the caller's all-reduce comes before this round
      for (const Inst* in : by_round[(size_t)r])
        if (b.units[(size_t)in->unit].mop < 0 && b.units[(size_t)in->unit].item < 0) { Launch x; x.phase = -2; out.push_back(x); }
      // serial chains: one block each, members in program order behind workgroup barriers (RK_SOLO; see solo_lat)
      part_lo = 0; part_cnt = -1;
      for (const Inst* in : by_round[(size_t)r]) {
        if (!(in_chain(in) && in->solo)) continue;
        const std::vector<int>& members = chains[(size_t)in->chain];
        if (&insts[(size_t)members[0]] != in) continue;
        phase = b.units[(size_t)in->unit].phase;
        const int ofs = (int)b.chain_tab.size();
        size_t lds = 64;
        b.chain_tab.push_back((int)members.size());
        if (opt.debug_plan) fprintf(stderr, "[ssn]   serial chain in round %d:", r);
        for (int mi : members) {
          const Inst& m = insts[(size_t)mi];
          const Unit& mu = b.units[(size_t)m.unit];
          if (mu.mop >= 0) {
            b.chain_tab.push_back(mu.mop);
            if (opt.debug_plan) fprintf(stderr, " k%d/%lld(s%d)", mops[(size_t)mu.mop].kind, (long long)mops[(size_t)mu.mop].len, m.sub);
          } else {
            const Item& it = items[(size_t)mu.item];      // (a transform: solo_lat admits nothing else)
            long long& ao = b.unit_arg[(size_t)m.unit];
            if (ao < 0) ao = (long long)b.put(&it.dft, sizeof it.dft);
            b.chain_tab.push_back(-(int)(ao / 16) - 1);
            lds = std::max(lds, dft_lds(it));
            if (opt.debug_plan) fprintf(stderr, " dft%d(s%d)", it.dft.kind, m.sub);
          }
          b.chain_tab.push_back(m.sub);
        }
        if (opt.debug_plan) fprintf(stderr, "\n");
        entry(ssn::RK_SOLO, 1, 1, lds, 3, (size_t)ofs);
      }
      // glue: one entry for all chunked micro-operators of the round
      const size_t map_begin = b.glue_map.size();
      for (const Inst* in : by_round[(size_t)r]) {
        const Unit& u = b.units[(size_t)in->unit];
        phase = u.phase;
        if (u.mop < 0) continue;
        if (in_chain(in) && in->solo) continue;
        const MOp& op = mops[(size_t)u.mop];
        if (op.kind == ssn::M_GATE || op.kind == ssn::M_ARGMAX_GATHER) continue;
        if (in_chain(in)) {
          const std::vector<int>& members = chains[(size_t)in->chain];
          if (&insts[(size_t)members[0]] != in) continue;                 // emitted with its chain's first member
          const int ofs = (int)b.chain_tab.size();
          if (opt.debug_plan) {
            fprintf(stderr, "[ssn]   chain in round %d (len %lld):", r, (long long)op.len);
            for (int mi : members) fprintf(stderr, " k%d", mops[(size_t)b.units[(size_t)insts[(size_t)mi].unit].mop].kind);
            fprintf(stderr, "\n");
          }
          b.chain_tab.push_back((int)members.size());
          for (int mi : members) { b.chain_tab.push_back(b.units[(size_t)insts[(size_t)mi].unit].mop); b.chain_tab.push_back(insts[(size_t)mi].sub); }
          const int blocks = (int)std::max<long long>(1, (op.len + ssn::GLUE_ROWS - 1) / ssn::GLUE_ROWS);
          for (int c = 0; c < blocks; ++c) b.glue_map.push_back(ssn::GlueBlock{-(ofs + 1), c});
          continue;
        }
        const long long per = kind_is(op.kind, ssn::MK_GLUE_ROW) ? ssn::GLUE_ROWS : ssn::GLUE_CHUNK;
        const int chunks = (int)std::max<long long>(1, (op.len + per - 1) / per);
        for (int c = 0; c < chunks; ++c) b.glue_map.push_back(ssn::GlueBlock{u.mop, c | (in->sub << 24)});
      }
      if (b.glue_map.size() > map_begin) entry(ssn::RK_GLUE, (int)(b.glue_map.size() - map_begin), 1, 64, 1, map_begin);
      for (const Inst* in : by_round[(size_t)r]) {
        const Unit& u = b.units[(size_t)in->unit];
        part_lo = in->lo; part_cnt = in->cnt;
        if (in_chain(in) && in->solo) continue;
        if (u.mop < 0 && u.item < 0) continue;        // (the exchange marker)
        if (u.mop >= 0) {
          const MOp& op = mops[(size_t)u.mop];
          if (op.kind == ssn::M_GATE) entry(ssn::RK_GATE, 1, 1, 64, 2, (size_t)u.mop);
          else if (op.kind == ssn::M_ARGMAX_GATHER) entry(ssn::RK_ARGMAX, 1, 1, 64, 2, (size_t)u.mop);
          continue;
        }
        const Item& it = items[(size_t)u.item];
        long long& ao = b.unit_arg[(size_t)in->unit];
        const RoundBody body = round_body(b, it, ao);
        if (body.kind >= 0) { entry(body.kind, body.gx, body.gy, body.lds, 0, (size_t)ao); continue; }
        Launch l; l.item = u.item; l.phase = u.phase;
        plain.push_back(l);
      }
      for (const Launch& l : plain) out.push_back(l);      // the plain launches first (ensemble arrays: the long ones), then the round's grid
      flush_entries();
      close();
    }
  }

  // access lists without the clock (timesteps planned together read it with an offset; it advances once, behind the last round)
  AccLists accesses_without_clock(const RoundBuild& b) const {
    AccLists acc(b.units.size());
    for (size_t u = 0; u < b.units.size(); ++u) { if (b.units[u].mop >= 0) micro_access(acc[u], mops[(size_t)b.units[u].mop], false); else acc[u] = b.units[u].acc; }
    return acc;
  }
  bool is_step_end(const Unit& u) const { return u.mop >= 0 && mops[(size_t)u.mop].kind == ssn::M_STEP_END; }

  // n timesteps of the units in `order`, software-pipelined: instance (u, s) takes the earliest round that its hazards against
  // the instances of timesteps s and s - 1 allow.  Returns the number of rounds.
  int place_steps(RoundBuild& b, const std::vector<int>& order, int n_steps, const AccLists& accs, std::vector<Inst>& all, Chains& chains) {
    all.reserve(order.size() * (size_t)n_steps);
    int nr = 0;
    const size_t per = order.size();
    for (int st = 0; st < n_steps; ++st)
      for (size_t q = 0; q < per; ++q) {
        const size_t lo = st > 0 ? (size_t)(st - 1) * per : 0;
        const int r = place(b, all, lo, order[q], accs, 0, chains);
        all.back().sub = st;
        nr = std::max(nr, r + 1);
      }
    return nr;
  }
  // the heavy instances of such a plan spread over their slack windows (`free_unit`: a unit without cost - the exchange of a sharded cycle plan)
  void balance(const RoundBuild& b, std::vector<Inst>& all, int nr, size_t per, const AccLists& accs, int free_unit) {
    if (opt.has(SSN_PLAN_NO_BALANCE)) return;
    balance_rounds(all, nr, per, [&](int x, int y) { return hazard(accs[(size_t)x], accs[(size_t)y]); },
                   [&](int u, double* us, double* lat, int* blocks) {
                     if (u == free_unit) { *us = 0.0; *lat = 0.0; *blocks = 0; return; }
                     unit_cost(b.units[(size_t)u].mop, b.units[(size_t)u].item, us, lat, blocks);
                   });
  }

  // (diagnostic) the chain of binding hazards behind the last instance of a pipelined plan: what its period is made of
  void print_critical_chain(const RoundBuild& b, const std::vector<Inst>& all, const AccLists& accs) const {
    if (all.empty()) return;        // (a model without a core - every operator time-batched - pipelines nothing: only the clock is stepped)
    size_t cur = 0;
    for (size_t i = 0; i < all.size(); ++i) if (all[i].round >= all[cur].round) cur = i;
    fprintf(stderr, "[ssn] critical chain (backwards from the last round):\n");
    for (int hop = 0; hop < 70 && all[cur].round > 0; ++hop) {
      const Unit& u = b.units[(size_t)all[cur].unit];
      if (u.mop >= 0) fprintf(stderr, "[ssn]   round %3d step %2d micro %d/%lld dst %lld\n", all[cur].round, all[cur].sub, mops[(size_t)u.mop].kind, (long long)mops[(size_t)u.mop].len, (long long)mops[(size_t)u.mop].dst);
      else if (u.item < 0) fprintf(stderr, "[ssn]   round %3d step %2d EXCHANGE\n", all[cur].round, all[cur].sub);
      else fprintf(stderr, "[ssn]   round %3d step %2d item %d type %d rows %d cols %d\n", all[cur].round, all[cur].sub, u.item, items[(size_t)u.item].type, items[(size_t)u.item].rows, items[(size_t)u.item].cols);
      size_t prev = cur;
      for (size_t v = cur; v-- > 0;)
        if (all[v].round == all[cur].round - 1 && hazard(accs[(size_t)all[cur].unit], accs[(size_t)all[v].unit])) { prev = v; break; }
      if (prev == cur)          // a chain member: its predecessor sits in the same round, in the same block
        for (size_t v = cur; v-- > 0;)
          if (all[v].round == all[cur].round && all[v].chain >= 0 && all[v].chain == all[cur].chain) { prev = v; break; }
      if (prev == cur) break;
      cur = prev;
    }
  }
  // (diagnostic, SSN_DEBUG_DEPS=<round>) what every instance of the steady-state rounds waits for in the round before it (diagnostic for in-launch dependencies)
  void print_deps(const RoundBuild& b, const std::vector<Inst>& all, const AccLists& accs) const {
    auto name = [&](const Inst& in) {
      const Unit& u = b.units[(size_t)in.unit];
      char buf[160];
      if (u.mop >= 0) snprintf(buf, sizeof buf, "micro k%d len %lld dst %lld", mops[(size_t)u.mop].kind, (long long)mops[(size_t)u.mop].len, (long long)mops[(size_t)u.mop].dst);
      else snprintf(buf, sizeof buf, "item %d type %d rows %d cols %d n %d", u.item, items[(size_t)u.item].type, items[(size_t)u.item].rows, items[(size_t)u.item].cols, items[(size_t)u.item].n);
      return std::string(buf);
    };
    const int r_lo = opt.debug_deps, r_hi = r_lo + 4;
    for (size_t i = 0; i < all.size(); ++i) {
      if (all[i].round < r_lo || all[i].round >= r_hi) continue;
      fprintf(stderr, "[ssn] deps: round %d step %d %s\n", all[i].round, all[i].sub, name(all[i]).c_str());
      for (size_t v = 0; v < all.size(); ++v) {
        if (v == i || all[v].round != all[i].round - 1) continue;
        const std::vector<Rng>& x = accs[(size_t)all[i].unit];
        const std::vector<Rng>& y = accs[(size_t)all[v].unit];
        bool raw = false, war = false, waw = false;
        for (const Rng& p : x) for (const Rng& q : y)
          if (p.space == q.space && p.lo < q.hi && q.lo < p.hi) { if (!p.w && q.w) raw = true; if (p.w && !q.w) war = true; if (p.w && q.w) waw = true; }
        if ((raw || war || waw) && (v < i)) fprintf(stderr, "[ssn] deps:     <- step %d %s%s%s%s\n", all[v].sub, name(all[v]).c_str(), raw ? " RAW" : "", war ? " WAR" : "", waw ? " WAW" : "");
      }
    }
  }
  void print_round_plan(const RoundBuild& b, const std::vector<Inst>& one, int n_rounds, int launches_unpipelined) const {
    fprintf(stderr, "[ssn] round plan: %zu units in %d rounds, %d launches per timestep; %d timesteps pipelined: %d rounds, %zu launches\n",
            b.units.size(), n_rounds, launches_unpipelined, steps_per_graph, graph_rounds, graph_list.size());
    for (const Launch& l : launch_list) {
      if (l.rl < 0) { const Item& it = items[(size_t)l.item]; fprintf(stderr, "[ssn]   plain item %d type %d rows %d cols %d n %d\n", l.item, it.type, it.rows, it.cols, it.n); continue; }
      const RoundLaunch& rl = round_launches[(size_t)l.rl];
      fprintf(stderr, "[ssn]   round %2d phase %d: %d blocks, %zu B LDS:", rl.round, l.phase, rl.n_blocks, rl.lds);
      for (int q = 0; q < rl.args.n; ++q) fprintf(stderr, " %d[%dx%d]", rl.args.e[q].kind, rl.args.e[q].gx, rl.args.e[q].gy);
      fprintf(stderr, "\n");
      for (const Inst& in : one)
        if (in.round == rl.round && b.units[(size_t)in.unit].mop >= 0) {
          const MOp& o = mops[(size_t)b.units[(size_t)in.unit].mop];
          fprintf(stderr, "[ssn]       micro %d/%lld dst %lld src %lld\n", o.kind, (long long)o.len, (long long)o.dst, (long long)o.src);
        }
    }
    for (const Launch& l : graph_list) {
      if (l.rl < 0) { fprintf(stderr, "[ssn]   pipelined: plain item %d type %d\n", l.item, items[(size_t)l.item].type); continue; }
      const RoundLaunch& rl = round_launches[(size_t)l.rl];
      fprintf(stderr, "[ssn]   pipelined round %3d: %6d blocks, %5zu B LDS:", rl.round, rl.n_blocks, rl.lds);
      for (int q = 0; q < rl.args.n; ++q) fprintf(stderr, " %d[%d]", rl.args.e[q].kind, rl.args.e[q].cnt);
      fprintf(stderr, "\n");
    }
  }

  // ---- one timestep: the eager / profiled / phased sequence --------------------------------------------------------
  int plan_one_step(RoundBuild& b, std::vector<Inst>& one) {
    int n_rounds = 0, phase1_base = 0;
    bool in_phase1 = false;
    AccLists acc_all(b.units.size());
    for (size_t u = 0; u < b.units.size(); ++u) acc_all[u] = b.units[u].acc;
    Chains chains_one;
    size_t phase1_from = 0;
    for (size_t u = 0; u < b.units.size(); ++u) {
      if (b.units[u].phase == 1 && !in_phase1) { in_phase1 = true; phase1_base = n_rounds; phase1_from = one.size(); }
      // (no chain across the exchange: a phase-1 instance only sees soft hazards with phase-1 instances; hard ones with all)
      int r = place(b, one, 0, (int)u, acc_all, in_phase1 ? phase1_base : 0, chains_one);
      if (in_phase1 && one.back().chain >= 0 && (size_t)chains_one[(size_t)one.back().chain][0] < phase1_from) {
        // joined a chain that started before the exchange: undo, take the first round of phase 1 instead
        chains_one[(size_t)one.back().chain].pop_back();
        const int r_own = r + (one.back().solo ? 1 : 0);        // (a serial member sat one round before its hard bound)
        one.back().chain = -1; one.back().solo = false; one.back().round = std::max(r_own, phase1_base);
        r = one.back().round;
      }
      n_rounds = std::max(n_rounds, r + 1);
    }
    launch_list.clear();
    emit(b, one, n_rounds, launch_list, chains_one);
    n_serial_chains = 0;
    for (size_t c = 0; c < chains_one.size(); ++c) if (chains_one[c].size() >= 2 && one[(size_t)chains_one[c][0]].solo) n_serial_chains += 1;
    launches_per_step = (int)launch_list.size();
    return n_rounds;
  }

  // ---- G timesteps software-pipelined: the sequence a step graph replays -------------------------------------------
  // Instance (u, s) takes the earliest round that its hazards against the instances of timesteps s and s - 1 allow
  // (a writer conflicts with itself one step earlier, so older steps are ordered transitively).  The recurrence of a
  // SLAM step runs through synapse states only: the long un-filtered chain of step s (two circular convolutions in
  // series) ends in filter updates that step s + 1 reads only to update other filters, so the head of step s + 1 -
  // the bandwidth-bound oscillators and encoder products - runs in the rounds where step s has one latency-bound
  // workgroup left.  Clock readers take the step number from StepCtx plus their own offset; the clock itself
  // advances once, behind the last round (k_advance).
  void plan_pipelined(RoundBuild& b) {
    graph_list.clear();
    graph_rounds = 0;
    const int G = steps_per_graph;
    if (phased || G <= 1 || opt.has(SSN_PLAN_NO_PIPELINE) || b.units.size() * (size_t)G > 40000) return;
    std::vector<int> keep;
    for (size_t u = 0; u < b.units.size(); ++u) if (!is_step_end(b.units[u])) keep.push_back((int)u);
    const AccLists acc_nc = accesses_without_clock(b);
    std::vector<Inst> all;
    Chains chains_all;
    const int nr = place_steps(b, keep, G, acc_nc, all, chains_all);
    if (opt.debug_plan) print_critical_chain(b, all, acc_nc);
    if (opt.debug_deps != PlanOptions::UNSET) print_deps(b, all, acc_nc);
    balance(b, all, nr, keep.size(), acc_nc, -1);
    emit(b, all, nr, graph_list, chains_all);
    graph_rounds = nr;
    launches_per_step = ((int)graph_list.size() + G - 1) / G;       // (average of the replayed sequence)
  }

  // ---- neuron-sharded models: what runs between two exchanges - the updates of timestep s (phase 1) and timestep s + 1 up to
  // its exchange (phase 0) - as ONE set of rounds.  A phase-0 operator of s + 1 waits only for the phase-1 operators whose
  // results it reads: table rows, the encoder products of tabulated inputs and whatever else does not hang on a filter state
  // start beside the filter updates, PES and Voja instead of behind them.  The clock is read with an offset (phase-0
  // instances: + 1) and advanced once behind the last round, as in the pipelined step graph.
  void plan_phase2(RoundBuild& b) {
    phase2_list.clear();
    if (!phased || opt.has(SSN_PLAN_NO_PIPELINE) || opt.phase2_sequential) return;
    const AccLists acc_p = accesses_without_clock(b);
    std::vector<Inst> comb;
    Chains chains_comb;
    int nr = 0;
    for (int ph = 1; ph >= 0; --ph)
      for (size_t u = 0; u < b.units.size(); ++u) {
        if (b.units[u].phase != ph || is_step_end(b.units[u])) continue;
        const int r = place(b, comb, 0, (int)u, acc_p, 0, chains_comb);
        comb.back().sub = ph == 0 ? 1 : 0;
        nr = std::max(nr, r + 1);
      }
    emit(b, comb, nr, phase2_list, chains_comb);
    if (opt.debug_plan) fprintf(stderr, "[ssn] phased plan: %zu launches per timestep apart (phase 0 + phase 1), %zu with the updates of s and the head of s + 1 planned together\n", launch_list.size(), phase2_list.size());
    launches_per_step = (int)phase2_list.size();
  }

  // ---- neuron-sharded models, pipelined over the exchange (round 4).  The plan above still starts every
  // timestep from an empty chip behind its exchange: ten rounds per timestep, none of them shared with another timestep.  Here
  // the exchange of timestep s is a unit of the plan like any other - it reads and writes the exchanged signal ranges, so the
  // operators that complete the partial sums come before it and their consumers (synapse filters, probes) behind it - and C
  // timesteps are placed together as in the unsharded step graph: what does not hang on the exchange of s (the head of
  // s + 1: tabulated inputs, encoder products, neuron updates of populations whose input is ready) shares rounds with the
  // tail of s.  The launch sequence is cut at the exchanges into C + 1 segments; the caller runs segment, all-reduce,
  // segment, ... (phase 3), the clock advances by C behind the last one.  SSN_CYCLE_STEPS: C (default 16; 0: off).
  void plan_cycle(RoundBuild& b) {
    cycle_segs.clear();
    cycle_steps = 0;
    const int C = opt.cycle_steps;
    if (!(phased && C > 1 && C <= 64 && !opt.has(SSN_PLAN_NO_PIPELINE) && (b.units.size() + 1) * (size_t)C <= 40000)) return;
    const int xu = (int)b.units.size();      // (the exchange's unit, below)
    std::vector<int> order;              // program order of one timestep with the exchange between its phases
    bool seen1 = false;
    for (int u = 0; u < xu; ++u) {
      if (is_step_end(b.units[(size_t)u])) continue;
      if (b.units[(size_t)u].phase == 1 && !seen1) { seen1 = true; order.push_back(xu); }
      order.push_back(u);
    }
    if (!seen1) return;
    {
      Unit x; x.phase = 0; x.writes = true;
      for (auto& r : exchange) x.acc.push_back(Rng{(const void*)sig, (int64_t)r.lo, (int64_t)r.hi, true});
      b.units.push_back(std::move(x));
      b.unit_arg.push_back(-1);
    }
    const AccLists acc_c = accesses_without_clock(b);
    std::vector<Inst> all;
    Chains chains_c;
    const int nr = place_steps(b, order, C, acc_c, all, chains_c);
    balance(b, all, nr, order.size(), acc_c, xu);
    if (opt.debug_plan) print_critical_chain(b, all, acc_c);
    std::vector<Launch> seq;
    emit(b, all, nr, seq, chains_c);
    cycle_segs.emplace_back();
    for (const Launch& l : seq) {
      if (l.phase == -2) { cycle_segs.emplace_back(); continue; }
      cycle_segs.back().push_back(l);
    }
    if ((int)cycle_segs.size() == C + 1) {
      cycle_steps = C;
      launches_per_step = ((int)(seq.size() - (size_t)C) + C - 1) / C;       // (average over the cycle)
      if (opt.debug_plan) {
        fprintf(stderr, "[ssn] sharded plan pipelined over the exchange: %d timesteps in %d rounds, %zu launches, segments:", C, nr, seq.size() - (size_t)C);
        for (auto& sg : cycle_segs) fprintf(stderr, " %zu", sg.size());
        fprintf(stderr, "\n");
      }
    } else {
      cycle_segs.clear();
    }
    b.units.pop_back();
    b.unit_arg.pop_back();
  }

  // device copies of the arena, the glue map and the chain table; the round entries get their pointers
  int upload_round_tables(const RoundBuild& b) {
    unsigned char* d_arena = nullptr; ssn::GlueBlock* d_map = nullptr; int* d_chain = nullptr;
    std::vector<unsigned char> arena = b.arena;      // (16 spare bytes: the tail of a body's arguments may be loaded as part of a whole 16-byte word)
    arena.resize(arena.size() + 16);
    CHK(dupload(&d_arena, arena));
    CHK(dupload(&d_map, b.glue_map));
    CHK(dupload(&d_chain, b.chain_tab));
    for (RoundLaunch& rl : round_launches) { rl.args.chain = d_chain; rl.args.arena = d_arena; }
    for (const Fix& f : b.fixes) {
      ssn::RoundEntry& e = round_launches[f.rl].args.e[f.entry];
      if (f.what == 0) e.args = d_arena + f.off;
      else if (f.what == 1) e.args = d_map + f.off;
      else if (f.what == 3) e.args = d_chain + f.off;
      else e.args = d_mops + f.off;
    }
    return SSN_OK;
  }

  int build_rounds(const std::vector<std::vector<MOp>>& programs_in, const std::vector<int>& item_prog) {
    std::vector<std::vector<MOp>> programs = programs_in;
    RoundBuild b;
    // rewrites of the operator list
    fold_pes_filters(programs, item_prog);
    CHK(fuse_product_neurons(programs, item_prog));
    // units (micro-operators cut at the other operators' range endpoints), the micro-operators on the device
    CHK(make_units(b, programs, item_prog));
    // launch sequences: one timestep; steps_per_graph timesteps pipelined; sharded models: what runs between two exchanges, and
    // cycle_steps timesteps pipelined over the exchange
    round_launches.clear();
    std::vector<Inst> one;
    const int n_rounds = plan_one_step(b, one);
    const int launches_unpipelined = launches_per_step;
    plan_pipelined(b);
    plan_phase2(b);
    plan_cycle(b);
    CHK(upload_round_tables(b));
    if (opt.debug_plan) print_round_plan(b, one, n_rounds, launches_unpipelined);
    return SSN_OK;
  }

  hipError_t launch_one(const Launch& l) {
    if (l.rl >= 0) { const RoundLaunch& rl = round_launches[(size_t)l.rl]; return ssn::launch_round<T>(stream, rl.args, rl.n_blocks, rl.lds); }
    return launch_item(items[(size_t)l.item]);
  }

  // Adjacent items of one kind with no data hazard between them share a launch (blockIdx.y selects the item).
  void merge_adjacent_items() {
    const int n = (int)items.size();
    auto xlds = [&](const Item& it) { return (size_t)it.cols * sizeof(T) <= 48 * 1024; };
    for (int i = 0; i < n; ++i) {
      Item& lead = items[(size_t)i];
      if (lead.merged || !(lead.type == IT_MATVEC || lead.type == IT_NEURONS || lead.type == IT_DFT || lead.type == IT_ENS || lead.type == IT_SPMV)) continue;
      if (lead.type == IT_ENS && (lead.dominant || lead.ens.defer)) continue;
      const int cap = lead.type == IT_ENS ? ssn::MAX_ENS_BATCH : ssn::MAX_BATCH;
      int k = 1;
      while (i + k < n && k < cap && items[(size_t)(i + k)].type == lead.type && items[(size_t)(i + k)].phase == lead.phase) {
        const Item& nx = items[(size_t)(i + k)];
        if (lead.type == IT_MATVEC && xlds(nx) != xlds(lead)) break;
        if (lead.type == IT_ENS && (nx.dominant || nx.ens.din != lead.ens.din || nx.ens.dout != lead.ens.dout || nx.ens.fast != lead.ens.fast)) break;
        bool indep = true;
        for (int d : item_deps[(size_t)(i + k)]) if (d >= i && d < i + k) indep = false;
        if (!indep) break;
        ++k;
      }
      lead.batch = k;
      for (int q = 1; q < k; ++q) items[(size_t)(i + q)].merged = true;
    }
    int launches = 0;
    for (auto& it : items) launches += it.merged ? 0 : 1;
    if (!core_empty) launches_per_step = launches - (can_fuse ? 1 : 0);
  }

  // Read / write sets of micro-operators and plan items (signal ranges, buffers and scratch memory by base pointer)
  void acc_sig(std::vector<Rng>& a, int64_t lo, int64_t len, bool w) const { if (len > 0) a.push_back(Rng{(const void*)sig, lo, lo + len, w}); }
  static void acc_ptr(std::vector<Rng>& a, const void* p, bool w) { if (p) a.push_back(Rng{p, 0, 1, w}); }
  // scattered destinations (decoded rows of an ensemble array) as runs of consecutive signals
  void acc_index_list(std::vector<Rng>& a, const void* dev_idx, bool w) const {
    for (auto& h : host_idx)
      if (h.first == dev_idx) {
        std::vector<int32_t> v(h.second.first, h.second.first + h.second.second);
        std::sort(v.begin(), v.end());
        for (size_t j = 0; j < v.size();) {
          size_t e = j + 1;
          while (e < v.size() && v[e] <= v[e - 1] + 1) ++e;
          acc_sig(a, v[j], (int64_t)v[e - 1] - v[j] + 1, w);
          j = e;
        }
      }
  }
  // (keep_empty: the operator's signal ranges of length 0 are listed too - hazard() then finds one inside another range)
  void micro_access(std::vector<Rng>& a, const MOp& op, bool with_clock = false, bool keep_empty = false) const {
    const void* clock = (const void*)d_ctx;
    auto range = [&](int64_t lo, int64_t len, bool w) { if (len > 0 || (keep_empty && len == 0)) a.push_back(Rng{(const void*)sig, lo, lo + len, w}); };
    switch (op.kind) {
      case ssn::M_FILL: range(op.dst, op.len, true); break;
      case ssn::M_TABLE: case ssn::M_ROW_IN: range(op.dst, op.len, true); if (with_clock) acc_ptr(a, clock, false); break;
      case ssn::M_AXPY_INC: case ssn::M_LOWPASS: range(op.src, op.len, false); range(op.dst, op.len, true); break;
      case ssn::M_AXPY_SET: range(op.src, op.len, false); range(op.dst, op.len, true); break;
      case ssn::M_LINCOMB: {
        auto it = lin_terms.find(op.p0);
        if (it != lin_terms.end()) for (auto& t : it->second) range(t.src, op.len, false);
        range(op.dst, op.len, true);
        break;
      }
      case ssn::M_MATVEC_INC: case ssn::M_MATVEC_SET: range(op.src, op.i0, false); range(op.dst, op.len, true); acc_ptr(a, op.p0, false); break;
      case ssn::M_GATE: range(op.src, 2 * op.len + 1, false); range(op.dst, op.len, true); break;
      case ssn::M_ARGMAX_GATHER: acc_ptr(a, op.p1, false); acc_ptr(a, op.p0, false); range(op.dst, op.len, true); break;
      case ssn::M_PROBE: case ssn::M_ROW_OUT: range(op.src, op.len, false); if (with_clock) acc_ptr(a, clock, false); break;
      case ssn::M_REDUCE_SET: case ssn::M_REDUCE_INC: acc_ptr(a, op.p0, false); range(op.dst, op.len, true); break;
      case ssn::M_ENS_FINISH: acc_ptr(a, op.p0, false); acc_index_list(a, op.p1, true); break;
      case ssn::M_STEP_END: if (with_clock) acc_ptr(a, clock, true); break;      // (item plan: the tail program is a join point anyway)
      default: break;
    }
  }
  void item_access(std::vector<Rng>& a, const Item& it) const {
    switch (it.type) {
      case IT_ENS:
        if (it.ens.direct) acc_index_list(a, (const void*)it.ens.didx, true);
        if (const TapSet* ts = it.taps) for (const ssn_tap_desc& t : ts->list) acc_sig(a, t.dst, t.count, true);
        acc_sig(a, it.ens.x_off, (int64_t)it.ens.K * it.ens.din, false);
        if (const DriveSet* ds = it.drv) {
          for (int32_t sx : ds->src) if (sx >= 0) acc_sig(a, sx, 1, false);
          acc_ptr(a, it.ens.drv_w, false);
        }
        for (int j = 0; j < it.ens.n_rec; ++j) acc_sig(a, it.ens.rec_src[j], it.ens.rec_len[j], false);      // (folded input terms)
        acc_ptr(a, it.ens.partials, true); acc_ptr(a, it.ens.V, true); acc_ptr(a, it.ens.R, true);
        acc_ptr(a, it.ens.enc, false); acc_ptr(a, it.ens.bias, false); acc_ptr(a, it.ens.dec, false);
        break;
      case IT_DFT:
        acc_sig(a, it.src - sig, it.cols, false); acc_sig(a, it.dst - sig, it.rows, true); acc_ptr(a, it.dft.tw, false);
        break;
      case IT_MATVEC: case IT_MATVEC_ORDERED:
        acc_sig(a, it.src - sig, it.cols, false); acc_ptr(a, it.Wm, false);
        if (it.dst >= sig && it.dst < sig + n_sig) acc_sig(a, it.dst - sig, it.rows, true); else acc_ptr(a, it.dst, true);
        break;
      case IT_GRID_LHS:
        acc_ptr(a, it.src, false); acc_ptr(a, it.aux0, false); acc_ptr(a, it.dst, true);
        break;
      case IT_GRID_GEMM: case IT_GRID_DOT:
        acc_ptr(a, it.src, false); acc_ptr(a, it.Wm, false); acc_ptr(a, it.dst, true);
        break;
      case IT_ARGMAX_PART:
        acc_ptr(a, it.src, false); acc_ptr(a, it.dst, true);
        break;
      case IT_SPMV:
        acc_sig(a, it.src - sig, it.cols, false); acc_ptr(a, it.Wm, false); acc_ptr(a, it.list, false); acc_ptr(a, it.count, false); acc_ptr(a, it.dst, true);
        break;
      case IT_NEURONS:
        acc_sig(a, it.src - sig, it.n, false); acc_sig(a, it.dst - sig, it.n, true); acc_ptr(a, it.V, true); acc_ptr(a, it.R, true);
        acc_ptr(a, it.list, true); acc_ptr(a, it.count, true);
        break;
      case IT_MATVEC_NEURONS:     // src: the current vector J (read unless the product sets), aux0: the product's input
        acc_sig(a, it.aux0 - sig, it.cols, false); acc_ptr(a, it.Wm, false);
        if (!it.set) acc_sig(a, it.src - sig, it.n, false);
        acc_sig(a, it.dst - sig, it.n, true); acc_ptr(a, it.V, true); acc_ptr(a, it.R, true);
        acc_ptr(a, it.list, true); acc_ptr(a, it.count, true);
        break;
      case IT_PES:
        acc_ptr(a, it.Wm, true); acc_sig(a, it.aux0 - sig, it.rows, false); acc_sig(a, it.aux1 - sig, it.cols, false);
        if (it.lp_dst) { acc_sig(a, it.lp_dst - sig, it.rows, true); acc_sig(a, it.lp_src - sig, it.rows, false); }
        break;
      case IT_VOJA:
        acc_ptr(a, it.Wm, true); acc_sig(a, it.src - sig, it.rows, false); acc_sig(a, it.aux0 - sig, it.cols, false); acc_sig(a, it.aux1 - sig, 1, false);
        acc_ptr(a, it.aux2, false);
        break;
      default: break;
    }
  }
  static bool hazard(const std::vector<Rng>& x, const std::vector<Rng>& y) {
    for (const Rng& p : x)
      for (const Rng& q : y)
        if (p.space == q.space && p.lo < q.hi && q.lo < p.hi && (p.w || q.w)) return true;
    return false;
  }

  // item_deps of the item plan (RAW, WAR and WAW hazards on earlier items).
  void analyse_dependencies(const std::vector<std::vector<MOp>>& programs, const std::vector<int>& item_prog) {
    std::vector<std::vector<Rng>> acc(items.size());
    int prog_i = 0;
    for (size_t i = 0; i < items.size(); ++i) {
      const Item& it = items[i];
      if (it.type == IT_PROGRAM) {
        for (const MOp& op : programs[(size_t)item_prog[(size_t)prog_i]]) micro_access(acc[i], op);
        ++prog_i;
      } else if (it.type == IT_VECOPS) {
        for (const MOp& op : vecops_host) micro_access(acc[i], op);
      } else {
        item_access(acc[i], it);
      }
    }
    item_deps.assign(items.size(), {});
    for (size_t i = 0; i < items.size(); ++i)
      for (size_t j = 0; j < i; ++j)
        if (hazard(acc[i], acc[j])) item_deps[i].push_back((int)j);
  }

  int init_bsig() {
    if (!bsig) return SSN_OK;
    CHK(upload(sig_init.data(), bsig, 1, n_sig, n_sig));
    for (int r = 1; r <= block; ++r)
      HIPCHK(hipMemcpyAsync(bsig + (size_t)r * n_sig, bsig, (size_t)n_sig * sizeof(T), hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return SSN_OK;
  }

  // Order and launches of a time-batched stage (ssn_stage_plan.hpp), once at plan(): neither depends on the block.
  void optimise_batch(std::vector<ssn::BatchOp<T>>& ops, std::vector<ssn::stage::Launch>& launches) {
    if (ops.size() >= 2 && !opt.no_batch_reorder) {
      std::vector<ssn::BatchOp<T>> out = ssn::stage::optimise(ops);
      if (opt.debug_plan) {
        fprintf(stderr, "[ssn] time-batched stage: %zu operators -> %zu\n", ops.size(), out.size());
        for (const ssn::BatchOp<T>& o : out) fprintf(stderr, "[ssn]   batch op kind %d dst %lld src %lld len %lld cols %d prev %d\n", o.kind, (long long)o.dst, (long long)o.src, (long long)o.len, o.cols, o.src_prev);
      }
      ops.swap(out);
    }
    launches = ssn::stage::pack(ops, !opt.has(SSN_PLAN_NO_STAGE_BATCH));
  }

  // One block of a stage: its launches in order, products of nothing but zeros left out (stage::ZeroMap).
  hipError_t run_batch(std::vector<ssn::BatchOp<T>>& ops, const std::vector<ssn::stage::Launch>& launches, int B, int64_t step0) {
    ssn::stage::ZeroMap<T> zeros(n_sig, !opt.no_zero_skip);
    auto note = [&](const ssn::BatchOp<T>& o) {              // effect of an operator that IS executed on the zero map
      bool z = false;
      if (o.kind == ssn::M_TABLE && !opt.no_zero_skip) {
        // the table's id from its slot: plan() makes p0 = d_tables + id and the (dst, len) that used to be searched for from the
        // same o.i[2], and every table operator has a signal range of its own - so the slot names the table the search found
        const size_t id = (size_t)((const ssn::TableSlot*)o.p0 - d_tables);
        z = id < table_idx_host.size() && table_is_zero((int)id, B, step0);
      }
      zeros.note(o, z);
    };
    for (const ssn::stage::Launch& l : launches) {
      for (int q = 0; q < l.count; ++q) { ops[(size_t)(l.first + q)].B = B; ops[(size_t)(l.first + q)].step0 = step0; }
      const ssn::BatchOp<T>& o = ops[(size_t)l.first];
      if (l.count > 1) {
        ssn::BatchOpList<T> list{};
        std::copy_n(&o, l.count, list.op);
        list.count = l.count;
        hipError_t e = ssn::launch_batch_elementwise<T>(stream, list);
        if (e != hipSuccess) return e;
        for (int q = 0; q < l.count; ++q) note(list.op[q]);      // (list order = program order of every thread)
        continue;
      }
      if (zeros.skippable(o)) {
        ++batch_skipped;
        if (o.kind == ssn::M_MATVEC_SET) {        // W @ 0: the result rows of the block are zero (an increment adds nothing)
          hipError_t e = hipMemset2DAsync(bsig + n_sig + o.dst, (size_t)n_sig * sizeof(T), 0, (size_t)o.len * sizeof(T), (size_t)B, stream);
          if (e != hipSuccess) return e;
        }
        zeros.note_skipped(o);
        continue;
      }
      hipError_t e = ssn::launch_batch_op<T>(stream, o);
      if (e != hipSuccess) return e;
      note(o);
    }
    return hipSuccess;
  }

  // Has the table no entry (index -1, or outside its range) for every timestep of this block?  Its rows are zeros then.
  bool table_is_zero(int id, int B, int64_t step0) const {
    const ssn::TableSlot& t = tables[(size_t)id];
    const std::vector<int32_t>& ix = table_idx_host[(size_t)id];
    for (int64_t st = step0; st < step0 + B; ++st) {
      const int64_t rel = st - t.first_step;
      if (rel >= 0 && rel < (int64_t)ix.size() && ix[(size_t)rel] >= 0) return false;
    }
    return true;
  }

  // ---- launching --------------------------------------------------------------------------
  hipError_t launch_item(const Item& it) {
    if (it.merged) return hipSuccess;               // its batch leader launched it
    const Item* g = &it;                            // (batch members are adjacent in `items`)
    switch (it.type) {
      case IT_PROGRAM: return ssn::launch_program<T>(stream, d_mops, d_progs + it.op_begin, 1, sig, d_ctx);
      case IT_VECOPS: return ssn::launch_vecops<T>(stream, d_mops + it.op_begin, it.op_count, it.n, sig, d_ctx);
      case IT_ENS: {
        if (it.batch > 1) {
          ssn::EnsBatch<T> b{};
          for (int q = 0; q < it.batch; ++q) b.a[q] = g[q].ens;
          return ssn::launch_ensarray_batch<T>(stream, b, it.batch);
        }
        return ssn::launch_ensarray<T>(stream, it.ens);
      }
      case IT_MATVEC: {
        ssn::MatvecBatch<T> b{};
        for (int q = 0; q < it.batch; ++q) b.a[q] = ssn::MatvecArgs<T>{g[q].Wm, g[q].src, g[q].dst, g[q].rows, g[q].cols, g[q].ld, g[q].set};
        return ssn::launch_matvec<T>(stream, b, it.batch);
      }
      case IT_MATVEC_ORDERED: return ssn::launch_matvec_ordered<T>(stream, it.Wm, it.src, it.dst, it.rows, it.cols, it.ld);
      case IT_FINISH: return ssn::launch_ens_finish<T>(stream, it.fin);
      case IT_DFT: {
        ssn::DftBatch b{};
        for (int q = 0; q < it.batch; ++q) b.a[q] = g[q].dft;
        return ssn::launch_dft<T>(stream, b, it.batch);
      }
      case IT_ARGMAX_PART: return ssn::launch_argmax_partial<T>(stream, it.src, (long long)it.rows, it.dst, it.n, std::max(1, it.seg));
      case IT_GRID_LHS: return ssn::launch_grid_lhs<T>(stream, it.src, it.aux0, it.ld, it.dst, it.cols, it.rows, it.cols / 2);
      case IT_GRID_DOT: return hipErrorInvalidValue;      // (planned only where the step runs as rounds)
      case IT_GRID_GEMM: return ssn::launch_gemm_nt<T>(stream, it.src, it.cols, it.Wm, it.ld, it.dst, it.n, it.rows, it.n, it.cols, std::max(1, it.seg));
      case IT_SPMV: {
        ssn::SpmvBatch<T> b{};
        for (int q = 0; q < it.batch; ++q)
          b.a[q] = ssn::SpmvArgs<T>{g[q].Wm, g[q].ld, g[q].src, g[q].cols, g[q].rows, g[q].dst, g[q].ld, g[q].n, g[q].list, g[q].count, g[q].seg, g[q].seg_len};
        return ssn::launch_spmv_partial<T>(stream, b, it.batch);
      }
      case IT_NEURONS: {
        ssn::NeuronsBatch<T> b{};
        for (int q = 0; q < it.batch; ++q)
          b.a[q] = ssn::NeuronsArgs<T>{g[q].np, g[q].src, g[q].dst, g[q].V, g[q].R, g[q].n, g[q].scalar, g[q].list, g[q].count};
        return ssn::launch_neurons<T>(stream, b, it.batch);
      }
      case IT_PES: return ssn::launch_pes<T>(stream, it.Wm, it.aux0, it.aux1, it.rows, it.cols, it.ld, it.scalar);
      case IT_VOJA: return ssn::launch_voja<T>(stream, it.Wm, it.src, it.aux0, it.aux1, it.aux2, it.rows, it.cols, it.ld, it.scalar);
    }
    return hipErrorInvalidValue;
  }

  hipError_t advance_clock(long long n) {
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, stream, d_ctx, n);
    return hipGetLastError();
  }

  // The event pairs of one profiled ssn_run_steps: pairs [0, used) of ev_pool are recorded; level 2 also notes the
  // plan-item type / index each pair belongs to.
  struct Timing { int level = 0; size_t used = 0; std::vector<int> types, items; };

  // One launch sequence, in order.  With `tm`, a launch runs between an event pair of its own: every launch at level 2,
  // the dominant kernel's at level 1.
  hipError_t launch_seq(const std::vector<Launch>& seq, Timing* tm = nullptr) {
    for (const Launch& l : seq) {
      const bool timed = tm && tm->used + 2 <= ev_pool.size() && (tm->level == 2 || (l.rl < 0 && items[(size_t)l.item].dominant));
      hipError_t e = timed ? hipEventRecord(ev_pool[tm->used], stream) : hipSuccess;
      if (e == hipSuccess) e = launch_one(l);
      if (e == hipSuccess && timed) e = hipEventRecord(ev_pool[tm->used + 1], stream);
      if (e != hipSuccess) return e;
      if (!timed) continue;
      if (tm->level == 2) {
        tm->types.push_back(l.rl >= 0 ? (int)IT_ROUND : items[(size_t)l.item].type);
        tm->items.push_back(l.rl >= 0 ? (int)items.size() + l.rl : l.item);
      }
      tm->used += 2;
    }
    return hipSuccess;
  }

  // `count` consecutive steps; fused = tail(s)+head(s+1) in one launch
  hipError_t launch_steps(int count, bool fused) {
    if (fused_defer) {                          // one k_ensarray per timestep; the clock advances once for the group
      for (int s = 0; s < count; ++s) {
        items[0].ens.sub = s;
        hipError_t e = launch_item(items[0]);
        if (e != hipSuccess) return e;
      }
      items[0].ens.sub = 0;
      return advance_clock(count);
    }
    if (round_mode) {
      if (count == steps_per_graph && !graph_list.empty()) {
        hipError_t e = launch_seq(graph_list);
        return e == hipSuccess ? advance_clock(count) : e;
      }
      for (int s = 0; s < count; ++s) { hipError_t e = launch_seq(launch_list); if (e != hipSuccess) return e; }
      return hipSuccess;
    }
    const int n_items = (int)items.size();
    for (int s = 0; s < count; ++s) {
      for (int i = 0; i < n_items; ++i) {
        const Item& it = items[i];
        hipError_t e = hipSuccess;
        if (fused && can_fuse && i == 0 && s > 0) continue;               // head already ran with the previous tail
        if (fused && can_fuse && i == n_items - 1 && s + 1 < count)
          e = ssn::launch_program<T>(stream, d_mops, d_progs + tail_begin, 2, sig, d_ctx);
        else
          e = launch_item(it);
        if (e != hipSuccess) return e;
      }
    }
    return hipSuccess;
  }

  // segment k of the pipelined sharded cycle (k = 0 .. cycle_steps); the clock advances behind the last one
  hipError_t launch_segment(int k) {
    hipError_t e = launch_seq(cycle_segs[(size_t)k]);
    return e == hipSuccess && k == cycle_steps ? advance_clock(cycle_steps) : e;
  }

  hipError_t launch_phase(int phase) {
    if (phase == 2) {          // updates of timestep s + timestep s + 1 up to its exchange
      if (round_mode && !phase2_list.empty()) {
        hipError_t e = launch_seq(phase2_list);
        return e == hipSuccess ? advance_clock(1) : e;
      }
      hipError_t e = launch_phase(1);
      return e == hipSuccess ? launch_phase(0) : e;
    }
    for (const Launch& l : launch_list) {
      if (l.phase != phase) continue;
      hipError_t e = launch_one(l);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }

  // What `body` launches on the compute stream becomes the graph `g` (which replaces the one it held).
  template <typename F>
  int capture_into(Graph& g, F body) {
    g.reset();
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const hipError_t e = body();
    const hipError_t e2 = hipStreamEndCapture(stream, &g.graph);        // (always: the stream must leave capture mode)
    HIPCHK(e);
    HIPCHK(e2);
    HIPCHK(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    return SSN_OK;
  }

  int capture() {
    if (phased) {             // one graph per half of the timestep
      if (fused_core || core_empty) return fail(SSN_EUNSUPPORTED, "neuron-sharded models run on the generic per-timestep plan");
      for (int h = 0; h < 3; ++h)          // [2]: phase 1 of a timestep + phase 0 of the next one in one launch
        CHK(capture_into(phase_graph[h], [&] { return launch_phase(h); }));
      return SSN_OK;
    }
    if (steps_per_graph <= 1 || fused_block) return SSN_OK;
    return capture_into(step_graph, [&] { return launch_steps(steps_per_graph, true); });
  }

  // The StepCtx the kernels kept against the host's count of timesteps; `before`: the call that reserves probe storage precedes.
  int check_device_state(const char* before) {
    ssn::StepCtx ctx;
    HIPCHK(hipMemcpy(&ctx, d_ctx, sizeof ctx, hipMemcpyDeviceToHost));
    if (ctx.step != steps_done) return fail(SSN_EHIP, "device step counter %lld != host %lld", (long long)ctx.step, (long long)steps_done);
    if (ctx.probe_overflow) return fail(SSN_EINVAL, "probe storage overflow: call ssn_reserve_probes before %s", before);
    return SSN_OK;
  }

  // Is `phase` (0 .. 3) what the entry point `fn` (ssn_run_phase, ssn_phase_async) may run next?
  int check_phase_order(const char* fn, int phase) {
    if (phase == 3) {
      if (!cycle_steps || !round_mode) return fail(SSN_EINVAL, "%s(3): this model has no pipelined cycle plan (ssn_cycle_steps() == 0)", fn);
      if (next_seg == 0 && next_phase != 0) return fail(SSN_EINVAL, "%s(3): a cycle starts at a timestep boundary (phase %d is due)", fn, next_phase);
      return SSN_OK;
    }
    if (next_seg != 0) return fail(SSN_EINVAL, "%s(%d): a pipelined cycle is under way (segment %d of %d is due)", fn, phase, next_seg, cycle_steps + 1);
    if ((phase == 2 ? 1 : phase) != next_phase) return fail(SSN_EINVAL, "%s(%d): phase %d is due", fn, phase, next_phase);
    return SSN_OK;
  }

  void advance_phase(int phase) {
    next_phase = phase == 0 ? 1 : (phase == 1 ? 0 : 1);
    if (phase >= 1) steps_done += 1;
  }

  // behind a segment of the pipelined cycle: true when it was the cycle's last one
  bool advance_segment() {
    if (++next_seg <= cycle_steps) return false;
    next_seg = 0;
    steps_done += cycle_steps;
    return true;
  }

  int run_phase(int phase) override {
    HIPCHK(hipSetDevice(device));
    if (!phased) return fail(SSN_EINVAL, "ssn_run_phase: the model has no exchange ranges (use ssn_run_steps)");
    if (next_seg == 0 && (phase < 0 || phase > 3)) return fail(SSN_EINVAL, "ssn_run_phase(%d): 0, 1 or 2 (= 1 followed by the next timestep's 0)", phase);
    CHK(check_phase_order("ssn_run_phase", phase));
    if (phase == 3) {            // the next segment of a pipelined cycle (eager launches; the caller exchanges between two segments)
      HIPCHK(launch_segment(next_seg));
      HIPCHK(hipStreamSynchronize(stream));
      return advance_segment() ? check_device_state("stepping") : SSN_OK;
    }
    HIPCHK(hipGraphLaunch(phase_graph[phase].exec, stream));
    HIPCHK(hipStreamSynchronize(stream));
    advance_phase(phase);
    if (phase >= 1 && (steps_done % 64 == 0 || steps_done == reserve_first + reserve_n))      // (a device -> host round trip: not on every timestep)
      return check_device_state("stepping");
    return SSN_OK;
  }

  int64_t cycle_len() override { return round_mode ? cycle_steps : 0; }

  int64_t exchange_size() override {
    int64_t n = 0;
    for (auto& r : exchange) n += r.hi - r.lo;
    return n;
  }

  // signal ranges of the exchange <-> one contiguous device buffer (a handful of ranges: one device copy each)
  hipError_t exchange_copy_async(void* buf, bool pack, hipStream_t st) {
    T* b = (T*)buf;
    for (auto& r : exchange) {
      const size_t bytes = (size_t)(r.hi - r.lo) * sizeof(T);
      hipError_t e = pack ? hipMemcpyAsync(b, sig + r.lo, bytes, hipMemcpyDeviceToDevice, st)
                          : hipMemcpyAsync(sig + r.lo, b, bytes, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return e;
      b += r.hi - r.lo;
    }
    return hipSuccess;
  }

  int exchange_copy(void* buf, bool pack) override {
    HIPCHK(hipSetDevice(device));
    HIPCHK(exchange_copy_async(buf, pack, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return SSN_OK;
  }

  // (Re)capture the graphs of stream-ordered stepping with the exchange copies of `buf` inside: [unpack] -> kernels -> [pack].
  int capture_async(void* buf) {
    auto with_exchange = [&](bool unpack, bool pack, auto launch) {
      hipError_t e = unpack && buf ? exchange_copy_async(buf, false, stream) : hipSuccess;
      if (e == hipSuccess) e = launch();
      if (e == hipSuccess && pack && buf) e = exchange_copy_async(buf, true, stream);
      return e;
    };
    for (int h = 0; h < 3; ++h)
      CHK(capture_into(async_graph[h], [&] { return with_exchange(h >= 1, h != 1, [&] { return launch_phase(h); }); }));
    cycle_graph.clear();
    if (cycle_steps && round_mode) {          // segment k: [unpack the sums of timestep k - 1] -> rounds -> [pack the partial sums of timestep k]
      cycle_graph.resize((size_t)cycle_steps + 1);
      for (int k = 0; k <= cycle_steps; ++k)
        CHK(capture_into(cycle_graph[(size_t)k], [&] { return with_exchange(k >= 1, k < cycle_steps, [&] { return launch_segment(k); }); }));
    }
    async_buf = buf;
    async_captured = true;
    return SSN_OK;
  }

  int phase_async(int phase, void* buf, hipStream_t ext) override {
    HIPCHK(hipSetDevice(device));
    if (!phased) return fail(SSN_EINVAL, "ssn_phase_async: the model has no exchange ranges (use ssn_run_steps)");
    if (phase == -1) {              // capture only: the graphs for this exchange buffer are built now, nothing is launched
      if (async_active) return fail(SSN_EINVAL, "ssn_phase_async(-1): a run is in flight (call ssn_phase_sync first)");
      HIPCHK(hipStreamSynchronize(stream));
      if (!async_captured || buf != async_buf) CHK(capture_async(buf));
      return SSN_OK;
    }
    if (next_seg == 0 && (phase < 0 || phase > 3)) return fail(SSN_EINVAL, "ssn_phase_async(%d): 0, 1, 2 (= 1 followed by the next timestep's 0) or 3 (next segment of a pipelined cycle)", phase);
    CHK(check_phase_order("ssn_phase_async", phase));
    if (!async_active) {
      HIPCHK(hipStreamSynchronize(stream));          // uploads / table updates issued on the simulator's own stream come first
      if (!async_captured || buf != async_buf) CHK(capture_async(buf));
      async_active = true;
    } else if (buf != async_buf) {
      return fail(SSN_EINVAL, "ssn_phase_async: the exchange buffer changed inside a run (call ssn_phase_sync first)");
    }
    async_stream = ext ? ext : stream;
    if (phase == 3) {
      HIPCHK(hipGraphLaunch(cycle_graph[(size_t)next_seg].exec, async_stream));
      advance_segment();
      return SSN_OK;
    }
    HIPCHK(hipGraphLaunch(async_graph[phase].exec, async_stream));
    advance_phase(phase);
    return SSN_OK;
  }

  int phase_sync(hipStream_t ext) override {
    HIPCHK(hipSetDevice(device));
    if (!phased) return fail(SSN_EINVAL, "ssn_phase_sync: the model has no exchange ranges");
    HIPCHK(hipStreamSynchronize(ext ? ext : stream));
    async_active = false;
    if (next_seg != 0) { const int due = next_seg; next_seg = 0; return fail(SSN_EINVAL, "ssn_phase_sync inside a pipelined cycle (segment %d of %d was due): the simulator's state is part-way through %d timesteps - reset it", due, cycle_steps + 1, cycle_steps); }
    return check_device_state("stepping");
  }

  // SSN_DEBUG_PLAN after a profile = 2 run: what every plan item / round launch took
  void print_profile() const {
    // diagnostic build (F32_EXTRA=-DSSN_PROGRAM_STAMPS): shader cycles each operator of each program took in the last timestep
    typedef int (*stamp_fn)(unsigned long long*, int);
    if (stamp_fn fn = (stamp_fn)dlsym(RTLD_DEFAULT, "ssn_debug_program_stamps")) {
      std::vector<unsigned long long> st(2048, 0);
      if (fn(st.data(), 2048) == 0)
        for (size_t p = 0; p < prog_descs.size(); ++p) {
          const ssn::ProgDesc& pd = prog_descs[p];
          if (pd.op_begin + pd.op_count > 1024) continue;
          unsigned long long prev = st[(size_t)(1024 + pd.op_begin)];
          fprintf(stderr, "[ssn] program %zu (%d ops) cycles per operator [kind/len:cycles]:", p, pd.op_count);
          for (int o = 0; o < pd.op_count; ++o) {
            const unsigned long long t = st[(size_t)(pd.op_begin + o)];
            if (!t) { fprintf(stderr, " %d/%lld:-", mops[(size_t)(pd.op_begin + o)].kind, (long long)mops[(size_t)(pd.op_begin + o)].len); continue; }
            fprintf(stderr, " %d/%lld:%lld", mops[(size_t)(pd.op_begin + o)].kind, (long long)mops[(size_t)(pd.op_begin + o)].len, (long long)(t - prev));
            prev = t;
          }
          fprintf(stderr, "\n");
        }
    }
    for (size_t i = 0; i < item_ms.size(); ++i)
      if (item_n[i]) {
        if (i < items.size()) fprintf(stderr, "[ssn] item %2zu type %2d batch %d: %8.2f us avg over %lld launches\n", i, items[i].type, items[i].batch,
                                      1e3 * item_ms[i] / item_n[i], (long long)item_n[i]);
        else fprintf(stderr, "[ssn] round launch %2zu (round %d, %d blocks): %8.2f us avg over %lld launches\n", i - items.size(),
                     round_launches[i - items.size()].round, round_launches[i - items.size()].n_blocks, 1e3 * item_ms[i] / item_n[i], (long long)item_n[i]);
      }
  }

  int run_steps(int64_t n, int profile) override {
    HIPCHK(hipSetDevice(device));
    if (phased) return fail(SSN_EINVAL, "a neuron-sharded model is stepped with ssn_run_phase (the caller exchanges between the phases)");
    if (n < 0) return fail(SSN_EINVAL, "negative step count");
    if (n == 0) return SSN_OK;
    int n_dom = 0;
    for (auto& it : items) n_dom += it.dominant ? 1 : 0;
    if (profile == 2 && (fused_block || core_empty)) profile = 1;
    Timing tm;
    tm.level = profile;
    if (profile) {
      // (launch_seq times at most launch_list.size() launches per timestep, or graph_list.size() per group; the budget stays
      //  what it was when item plans had no launch_list: all items, plus the round plan's launches)
      const size_t per_step = profile == 2 ? items.size() + (round_mode ? launch_list.size() : 0) : (size_t)std::max(1, n_dom);
      const size_t need = fused_block ? (size_t)(2 * (n / std::max(1, block) + 2)) : (size_t)(2 * n * (int)per_step);
      if (need > 400000) return fail(SSN_EINVAL, "profile run too long (%lld steps): at most 200000 timed launches", (long long)n);
      while (ev_pool.size() < need) {
        hipEvent_t ev;
        HIPCHK(hipEventCreate(&ev));
        ev_pool.push_back(ev);
      }
    }
    HIPCHK(hipEventRecord(ev_run0, stream));
    int64_t done = 0;
    while (done < n) {
      // one block: [pre stage, batched] -> core, one timestep at a time -> [post stage, batched]
      const int64_t B = bsig ? std::min<int64_t>(block, n - done) : (n - done);
      const int64_t step0 = steps_done + done;
      if (bsig) {
        hipLaunchKernelGGL(k_set_block, dim3(1), dim3(1), 0, stream, d_ctx, (long long)step0);
        HIPCHK(hipGetLastError());
        HIPCHK(run_batch(pre_ops, pre_launches, (int)B, step0));
      }
      if (fused_defer) HIPCHK(ssn::launch_ens_finish<T>(stream, fin_begin));
      if (fused_block) {
        const bool timed = profile && B == block && tm.used + 2 <= ev_pool.size();
        blk.B = (int)B;
        if (blk.P > 1)      // every exchange word back to the sentinel: the kernel boundary is the members' only common barrier
          HIPCHK(hipMemsetD32Async((hipDeviceptr_t)blk.xslots, (int)ssn::BLOCK_XCHG_SENTINEL, (size_t)3 * blk.K * 64, stream));
        if (timed) HIPCHK(hipEventRecord(ev_pool[tm.used], stream));
        HIPCHK(ssn::launch_ens_block<T>(stream, blk));
        if (timed) { HIPCHK(hipEventRecord(ev_pool[tm.used + 1], stream)); tm.used += 2; }
        HIPCHK(advance_clock(B));
      } else if (core_empty) {
        // nothing is stepped one timestep at a time (purely feed-forward model): just advance the clock
        HIPCHK(advance_clock(B));
      } else if (profile) {
        // timed launches (2: every launch between its own event pair, 1: the dominant kernel's) - plain eager launches, no
        // graph and no fused programs
        int64_t s = 0;
        if (profile == 2 && round_mode && !graph_list.empty())
          for (; s + steps_per_graph <= B; s += steps_per_graph) {      // the pipelined sequence a step graph replays, launch by launch
            HIPCHK(launch_seq(graph_list, &tm));
            HIPCHK(advance_clock(steps_per_graph));
          }
        for (; s < B; ++s) {
          HIPCHK(launch_seq(launch_list, &tm));
          if (fused_defer) HIPCHK(advance_clock(1));
        }
      } else {
        int64_t left = B;
        if (step_graph.exec)
          for (; left >= steps_per_graph; left -= steps_per_graph) HIPCHK(hipGraphLaunch(step_graph.exec, stream));
        if (left > 0) HIPCHK(launch_steps((int)left, true));
      }
      if (fused_defer) HIPCHK(ssn::launch_ens_finish<T>(stream, fin_flush));
      if (bsig) {
        HIPCHK(run_batch(post_ops, post_launches, (int)B, step0));
        HIPCHK(hipMemcpyAsync(bsig, bsig + (size_t)B * n_sig, (size_t)n_sig * sizeof(T), hipMemcpyDeviceToDevice, stream));
      }
      done += B;
    }
    HIPCHK(hipEventRecord(ev_run1, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (size_t j = 0; j < tm.used; j += 2) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev_pool[j], ev_pool[j + 1]));
      if (profile == 2) {
        const int ty = tm.types[j / 2];
        type_ms[ty] += ms;
        type_launches[ty] += 1;
        if (item_ms.size() != items.size() + round_launches.size()) { item_ms.assign(items.size() + round_launches.size(), 0.0); item_n.assign(items.size() + round_launches.size(), 0); }
        item_ms[(size_t)tm.items[j / 2]] += ms; item_n[(size_t)tm.items[j / 2]] += 1;
        continue;
      }
      dom_ms += ms;
      dom_launches += 1;
    }
    if (profile == 2 && opt.debug_plan) print_profile();
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev_run0, ev_run1));
    last_run_ms = ms;
    steps_done += n;
    CHK(check_device_state("ssn_run_steps"));
    if (fused_block && blk.P > 1) {
      int xe = 0;
      HIPCHK(hipMemcpy(&xe, blk.xerr, sizeof xe, hipMemcpyDeviceToHost));
      if (xe) return fail(SSN_EHIP, "split ensembles: a member workgroup waited too long for a partner's sums (are all %d workgroups "
                                    "resident together? flag 1073741824 needs the GPU for this process alone)", blk.K * blk.P);
    }
    return SSN_OK;
  }

  int reset() override {
    HIPCHK(hipSetDevice(device));
    if (async_active) {          // phase graphs may still be queued on the caller's stream: they come first
      HIPCHK(hipStreamSynchronize(async_stream ? async_stream : stream));
      async_active = false;
    }
    HIPCHK(hipStreamSynchronize(stream));
    CHK(upload(sig_init.data(), sig, 1, n_sig, n_sig));
    for (auto& b : bufs)
      if (b.keep) CHK(upload_buf(b, b.host.data()));
    HIPCHK(hipMemset(d_ctx, 0, sizeof(ssn::StepCtx)));
    CHK(init_bsig());
    steps_done = 0;
    next_phase = 0;
    next_seg = 0;
    reserve_first = reserve_n = 0;
    for (auto& s : pslots) { s.base_slot = 0; s.capacity = 0; }
    if (!pslots.empty()) HIPCHK(hipMemcpy(d_pslots, pslots.data(), pslots.size() * sizeof(ssn::ProbeSlot), hipMemcpyHostToDevice));
    dom_launches = 0; dom_ms = 0.0;
    for (int t = 0; t < N_ITEM_TYPES; ++t) { type_ms[t] = 0.0; type_launches[t] = 0; }
    if (fused_block && blk.slot_stats) HIPCHK(hipMemset(blk.slot_stats, 0, 16));
    return SSN_OK;
  }

  int set_table(int id, const double* rows, const void* rows_dev, int64_t n_rows, int64_t width,
                const int32_t* idx, int64_t n_idx, int64_t first_step) override {
    HIPCHK(hipSetDevice(device));
    if (async_active) return fail(SSN_EINVAL, "a stream-ordered run is in flight on the caller's stream: call ssn_phase_sync first");
    if (id < 0 || id >= (int)tables.size()) return fail(SSN_EINVAL, "table id %d out of range", id);
    if (width != tables[id].width) return fail(SSN_EINVAL, "table %d is %lld wide, got %lld", id, (long long)tables[id].width, (long long)width);
    if (n_rows < 0 || n_idx < 0 || (!idx && n_idx)) return fail(SSN_EINVAL, "bad table arguments");
    for (int64_t i = 0; i < n_idx; ++i)
      if (idx[i] >= n_rows) return fail(SSN_EINVAL, "table row index %d >= n_rows %lld", idx[i], (long long)n_rows);
    HIPCHK(hipStreamSynchronize(stream));
    const int64_t need = std::max<int64_t>(1, n_rows * width);
    CHK(table_rows[id].grow(*this, need * (int64_t)sizeof(T)));
    CHK(table_idx[id].grow(*this, n_idx * 4));
    if (rows_dev) HIPCHK(hipMemcpy(table_rows[id].p, rows_dev, (size_t)(n_rows * width) * sizeof(T), hipMemcpyDeviceToDevice));
    else if (n_rows) CHK(upload(rows, (T*)table_rows[id].p, n_rows, width, width));
    if (n_idx) HIPCHK(hipMemcpy(table_idx[id].p, idx, (size_t)n_idx * 4, hipMemcpyHostToDevice));
    if (table_idx_host.size() < tables.size()) table_idx_host.resize(tables.size());
    table_idx_host[(size_t)id].assign(idx, idx + n_idx);
    tables[id] = ssn::TableSlot{table_rows[id].p, (int*)table_idx[id].p, n_rows, width, n_idx, first_step};
    HIPCHK(hipMemcpy(d_tables + id, &tables[id], sizeof(ssn::TableSlot), hipMemcpyHostToDevice));
    return SSN_OK;
  }

  // Rows already in the simulator's type (the caller converted them): pure DMA into the inactive buffer set on the copy
  // stream - no kernel, so it proceeds while a compute kernel owns every CU, and any host thread may call it during ssn_run_steps.
  int stage_table(int id, const void* rows_t, int64_t n_rows, int64_t width, const int32_t* idx, int64_t n_idx, int64_t first_step) override {
    HIPCHK(hipSetDevice(device));
    if (id < 0 || id >= (int)tables.size()) return fail(SSN_EINVAL, "table id %d out of range", id);
    if (width != tables[id].width) return fail(SSN_EINVAL, "table %d is %lld wide, got %lld", id, (long long)tables[id].width, (long long)width);
    if (n_rows < 0 || n_idx < 0 || (!idx && n_idx) || (!rows_t && n_rows)) return fail(SSN_EINVAL, "bad table arguments");
    for (int64_t i = 0; i < n_idx; ++i)
      if (idx[i] >= n_rows) return fail(SSN_EINVAL, "table row index %d >= n_rows %lld", idx[i], (long long)n_rows);
    std::lock_guard<std::mutex> lock(stage_mutex);
    if (!copy_stream) HIPCHK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    Staged& g = staged[(size_t)id];
    g.valid = false;
    const int64_t need = std::max<int64_t>(1, n_rows * width);
    CHK(g.rows.grow(*this, need * (int64_t)sizeof(T)));
    CHK(g.idx.grow(*this, n_idx * 4));
    if (n_rows) HIPCHK(hipMemcpyAsync(g.rows.p, rows_t, (size_t)(n_rows * width) * sizeof(T), hipMemcpyHostToDevice, copy_stream));
    if (n_idx) HIPCHK(hipMemcpyAsync(g.idx.p, idx, (size_t)n_idx * 4, hipMemcpyHostToDevice, copy_stream));
    HIPCHK(hipStreamSynchronize(copy_stream));          // (the host arrays are the caller's again)
    g.n_rows = n_rows; g.width = width; g.n_idx = n_idx; g.first_step = first_step;
    g.idx_host.assign(idx, idx + n_idx);
    g.valid = true;
    return SSN_OK;
  }

  int commit_tables() override {
    HIPCHK(hipSetDevice(device));
    if (async_active) return fail(SSN_EINVAL, "a stream-ordered run is in flight on the caller's stream: call ssn_phase_sync first");
    std::lock_guard<std::mutex> lock(stage_mutex);
    bool any = false;
    for (auto& g : staged) any = any || g.valid;
    if (!any) return SSN_OK;
    HIPCHK(hipStreamSynchronize(stream));              // the run that read the current set has ended
    if (table_idx_host.size() < tables.size()) table_idx_host.resize(tables.size());
    for (size_t id = 0; id < staged.size(); ++id) {
      Staged& g = staged[id];
      if (!g.valid) continue;
      g.rows.swap(table_rows[id]); g.idx.swap(table_idx[id]);
      table_idx_host[id].swap(g.idx_host);
      tables[id] = ssn::TableSlot{table_rows[id].p, (int*)table_idx[id].p, g.n_rows, g.width, g.n_idx, g.first_step};
      g.valid = false;
    }
    HIPCHK(hipMemcpy(d_tables, tables.data(), tables.size() * sizeof(ssn::TableSlot), hipMemcpyHostToDevice));
    return SSN_OK;
  }

  int reserve_probes(int64_t n) override {
    HIPCHK(hipSetDevice(device));
    if (async_active) return fail(SSN_EINVAL, "a stream-ordered run is in flight on the caller's stream: call ssn_phase_sync first");
    HIPCHK(hipStreamSynchronize(stream));
    reserve_first = steps_done;
    reserve_n = n;
    for (size_t p = 0; p < pslots.size(); ++p) {
      const int64_t every = probes[p].every;
      const int64_t base = steps_done / every;
      const int64_t cap = (steps_done + n) / every - base;
      const int64_t bytes = std::max<int64_t>(1, cap * probes[p].width) * (int64_t)sizeof(T);
      CHK(probe_store[p].grow(*this, bytes));
      pslots[p].data = probe_store[p].p;
      pslots[p].base_slot = base;
      pslots[p].capacity = cap;
    }
    if (!pslots.empty()) HIPCHK(hipMemcpy(d_pslots, pslots.data(), pslots.size() * sizeof(ssn::ProbeSlot), hipMemcpyHostToDevice));
    return SSN_OK;
  }

  int64_t probe_count(int id) override {
    if (id < 0 || id >= (int)pslots.size()) return -1;
    const int64_t every = probes[id].every;
    return std::min<int64_t>(pslots[id].capacity, steps_done / every - pslots[id].base_slot);
  }

  int read_probe(int id, double* dst, void* dst_dev, int64_t first, int64_t count) override {
    HIPCHK(hipSetDevice(device));
    if (async_active) return fail(SSN_EINVAL, "a stream-ordered run is in flight on the caller's stream: call ssn_phase_sync first");
    if (id < 0 || id >= (int)pslots.size()) return fail(SSN_EINVAL, "probe id %d out of range", id);
    if (first < 0 || count < 0 || first + count > probe_count(id))
      return fail(SSN_EINVAL, "probe %d holds %lld samples, asked for [%lld,+%lld)", id, (long long)probe_count(id), (long long)first, (long long)count);
    const int64_t w = probes[id].width;
    const T* src = (const T*)pslots[id].data + first * w;
    if (dst_dev) {
      HIPCHK(hipMemcpyAsync(dst_dev, src, (size_t)(count * w) * sizeof(T), hipMemcpyDeviceToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
      return SSN_OK;
    }
    return download(src, dst, count, w, w);
  }

  int rw_signal(int64_t off, int64_t count, double* dst, const double* src) override {
    HIPCHK(hipSetDevice(device));
    if (async_active) return fail(SSN_EINVAL, "a stream-ordered run is in flight on the caller's stream: call ssn_phase_sync first");
    CHK(check_range(off, count, "signal access"));
    if (!dst) {
      CHK(upload(src, sig + off, 1, count, count));
      return bsig ? upload(src, bsig + off, 1, count, count) : SSN_OK;
    }
    CHK(download(sig + off, dst, 1, count, count));
    if (bsig) {                       // signals of the batched stages live in the block buffer (row 0 = latest)
      std::vector<double> tmp((size_t)count);
      CHK(download(bsig + off, tmp.data(), 1, count, count));
      for (int64_t i = 0; i < count; ++i) if (batched_mask[(size_t)(off + i)]) dst[i] = tmp[(size_t)i];
    }
    return SSN_OK;
  }

  int rw_buffer(int id, double* dst, const double* src, int64_t count) override {
    HIPCHK(hipSetDevice(device));
    if (async_active) return fail(SSN_EINVAL, "a stream-ordered run is in flight on the caller's stream: call ssn_phase_sync first");
    if (id < 0 || id >= (int)bufs.size()) return fail(SSN_EINVAL, "buffer id %d out of range", id);
    Buf& b = bufs[id];
    if (b.kind != SSN_BUF_REAL || count != b.count) return fail(SSN_EINVAL, "buffer %d: real buffer of %lld elements expected", id, (long long)b.count);
    if (dst) return download_buf(b, dst);
    if (b.packed == 2) return fail(SSN_EUNSUPPORTED, "buffer %d: the refractory times of a LIF ensemble array are packed with its voltages; write the voltage buffer", id);
    return upload_buf(b, src);
  }

  int counters(ssn_counters* out) override {
    out->n_steps = steps_done;
    out->launches_per_step = launches_per_step;
    out->dominant_launches = dom_launches;
    out->dominant_ms_total = dom_ms;
    out->dominant_bytes_per_launch = dom_bytes;
    out->dominant_units_per_launch = dom_units;
    out->last_run_ms = last_run_ms;
    out->device_bytes = device_bytes;
    out->block_tpb = fused_block ? blk.tpb : 0;
    out->block_npt = fused_block ? blk.npt : 0;
    out->block_enc_lds = fused_block ? blk.enc_lds : 0;
    out->block_threads = fused_block ? blk.threads : 0;
    out->block_members = fused_block ? std::max(1, blk.P) : 0;
    out->batch_products_skipped = batch_skipped;
    out->block_slots = 0; out->block_slots_silent = 0;
    out->fused_populations = n_fused_populations; out->serial_chains = n_serial_chains;
    if (fused_block && blk.slot_stats) {
      unsigned long long ss[2] = {0, 0};
      hipSetDevice(device);
      if (hipMemcpy(ss, blk.slot_stats, sizeof ss, hipMemcpyDeviceToHost) == hipSuccess) { out->block_slots = (int64_t)ss[0]; out->block_slots_silent = (int64_t)ss[1]; }
    }
    out->fft_transforms = 0; out->fft_bluestein = 0;
    for (auto& it : items) if (it.type == IT_DFT) { out->fft_transforms += 1; out->fft_bluestein += it.dft.M > 0 ? 1 : 0; }
    return SSN_OK;
  }

  int kernel_times(ssn_kernel_time* out, int capacity) override {
    static const char* names[N_ITEM_TYPES] = {"k_program", "k_ensarray", "k_matvec", "k_neurons", "k_pes", "k_voja", "k_matvec_ordered",
                                              "k_ens_finish", "k_spmv_partial", "k_dft", "k_vecops", "k_grid_lhs", "k_gemm_nt_mfma_f32",
                                              "k_argmax_partial", "k_round", "", "", ""};
    int n = 0;
    for (int t = 0; t < N_ITEM_TYPES; ++t) {
      if (!type_launches[t]) continue;
      if (n < capacity) {
        snprintf(out[n].name, sizeof out[n].name, "%s", names[t]);
        out[n].launches = type_launches[t];
        out[n].ms_total = type_ms[t];
      }
      ++n;
    }
    return n;
  }

  int64_t n_steps() override { return steps_done; }

  int buffer_view(int id, ssn::BufView* out) override {
    if (async_active) return fail(SSN_EINVAL, "a stream-ordered run is in flight on the caller's stream: call ssn_phase_sync first");
    if (id < 0 || id >= (int)bufs.size()) return fail(SSN_EINVAL, "buffer id %d out of range", id);
    const Buf& b = bufs[id];
    if (b.kind != SSN_BUF_REAL || !b.shaped || !b.d) return fail(SSN_EINVAL, "buffer %d is not a matrix of reals", id);
    if (b.perm || b.dec_DP || b.packed) return fail(SSN_EUNSUPPORTED, "buffer %d belongs to an ensemble array (packed or re-ordered on the device)", id);
    out->d = b.d; out->dtype = sizeof(T) == 4 ? SSN_F32 : SSN_F64; out->device = device; out->stream = stream;
    out->rows = b.rows; out->cols = b.cols; out->ld = b.ld; out->transposed = b.transposed ? 1 : 0; out->ldt = b.ldt;
    return SSN_OK;
  }
};

template <typename T>
int create_sim(const ssn_model_desc* desc, ssn_sim** out) {
  auto s = std::make_unique<Sim<T>>(desc);
  int rc = s->create(desc);
  if (rc != SSN_OK) return rc;
  *out = s.release();
  return SSN_OK;
}

}  // namespace

namespace ssn {
int sim_buffer_view(ssn_sim* sim, int id, BufView* out) { return sim && out ? sim->buffer_view(id, out) : fail(SSN_EINVAL, "null simulator"); }
}  // namespace ssn

extern "C" {

int ssn_create(const ssn_model_desc* desc, ssn_sim** out) {
  if (!desc || !out) return fail(SSN_EINVAL, "null argument");
  *out = nullptr;
  if (desc->abi_version != SSN_ABI_VERSION) return fail(SSN_EINVAL, "ABI version %d != %d", desc->abi_version, SSN_ABI_VERSION);
  if (desc->flags & ~SSN_PLAN_ALL_FLAGS)
    return fail(SSN_EINVAL, "flags %d: the bits %d are no plan switch (ssn_plan_flag in ssn.h)", desc->flags, desc->flags & ~SSN_PLAN_ALL_FLAGS);
  if (desc->n_signals <= 0 || !desc->signal_init || desc->n_ops <= 0 || !desc->ops || desc->dt <= 0)
    return fail(SSN_EINVAL, "empty or inconsistent model description");
  int ndev = 0;
  const hipError_t dev_err = hipGetDeviceCount(&ndev);
  if (dev_err != hipSuccess || ndev <= 0)
    return fail(SSN_EHIP, "no HIP device available (there is no CPU fallback): hipGetDeviceCount -> %s, %d devices", hipGetErrorString(dev_err), ndev);
  if (desc->device < 0 || desc->device >= ndev) return fail(SSN_EINVAL, "device %d out of range (%d devices)", desc->device, ndev);
  if (desc->dtype == SSN_F32) return create_sim<float>(desc, out);
  if (desc->dtype == SSN_F64) return create_sim<double>(desc, out);
  return fail(SSN_EINVAL, "unknown dtype %d", desc->dtype);
}

void ssn_destroy(ssn_sim* sim) { delete sim; }
int ssn_reset(ssn_sim* sim) { return sim ? sim->reset() : fail(SSN_EINVAL, "null simulator"); }
int ssn_set_table(ssn_sim* sim, int32_t id, const double* rows, int64_t n_rows, int64_t width, const int32_t* idx,
                  int64_t n_idx, int64_t first_step) {
  if (!sim || (!rows && n_rows)) return fail(SSN_EINVAL, "null argument");
  return sim->set_table(id, rows, nullptr, n_rows, width, idx, n_idx, first_step);
}
int ssn_set_table_device(ssn_sim* sim, int32_t id, const void* rows_dev, int64_t n_rows, int64_t width,
                         const int32_t* idx, int64_t n_idx, int64_t first_step) {
  if (!sim || !rows_dev) return fail(SSN_EINVAL, "null argument");
  return sim->set_table(id, nullptr, rows_dev, n_rows, width, idx, n_idx, first_step);
}
int ssn_stage_table(ssn_sim* sim, int32_t id, const void* rows_t, int64_t n_rows, int64_t width, const int32_t* idx, int64_t n_idx, int64_t first_step) {
  if (!sim) return fail(SSN_EINVAL, "null simulator");
  return sim->stage_table(id, rows_t, n_rows, width, idx, n_idx, first_step);
}
int ssn_commit_tables(ssn_sim* sim) { return sim ? sim->commit_tables() : fail(SSN_EINVAL, "null simulator"); }
int ssn_reserve_probes(ssn_sim* sim, int64_t n) { return sim ? sim->reserve_probes(n) : fail(SSN_EINVAL, "null simulator"); }
int ssn_run_steps(ssn_sim* sim, int64_t n, int32_t profile) { return sim ? sim->run_steps(n, profile) : fail(SSN_EINVAL, "null simulator"); }
int ssn_read_probe(ssn_sim* sim, int32_t id, double* dst, int64_t first, int64_t count) {
  if (!sim || (!dst && count)) return fail(SSN_EINVAL, "null argument");
  return sim->read_probe(id, dst, nullptr, first, count);
}
int ssn_read_probe_device(ssn_sim* sim, int32_t id, void* dst_dev, int64_t first, int64_t count) {
  if (!sim || !dst_dev) return fail(SSN_EINVAL, "null argument");
  return sim->read_probe(id, nullptr, dst_dev, first, count);
}
int64_t ssn_probe_count(ssn_sim* sim, int32_t id) { return sim ? sim->probe_count(id) : -1; }
int ssn_read_signal(ssn_sim* sim, int64_t off, int64_t count, double* dst) {
  if (!sim || !dst) return fail(SSN_EINVAL, "null argument");
  return sim->rw_signal(off, count, dst, nullptr);
}
int ssn_write_signal(ssn_sim* sim, int64_t off, int64_t count, const double* src) {
  if (!sim || !src) return fail(SSN_EINVAL, "null argument");
  return sim->rw_signal(off, count, nullptr, src);
}
int ssn_read_buffer(ssn_sim* sim, int32_t id, double* dst, int64_t count) {
  if (!sim || !dst) return fail(SSN_EINVAL, "null argument");
  return sim->rw_buffer(id, dst, nullptr, count);
}
int ssn_write_buffer(ssn_sim* sim, int32_t id, const double* src, int64_t count) {
  if (!sim || !src) return fail(SSN_EINVAL, "null argument");
  return sim->rw_buffer(id, nullptr, src, count);
}
int ssn_get_counters(ssn_sim* sim, ssn_counters* out) {
  if (!sim || !out) return fail(SSN_EINVAL, "null argument");
  return sim->counters(out);
}
int ssn_run_phase(ssn_sim* sim, int32_t phase) { return sim ? sim->run_phase(phase) : fail(SSN_EINVAL, "null simulator"); }
int64_t ssn_exchange_size(ssn_sim* sim) { return sim ? sim->exchange_size() : -1; }
int64_t ssn_cycle_steps(ssn_sim* sim) { return sim ? sim->cycle_len() : -1; }
int ssn_exchange_pack(ssn_sim* sim, void* dst_dev) {
  if (!sim || !dst_dev) return fail(SSN_EINVAL, "null argument");
  return sim->exchange_copy(dst_dev, true);
}
int ssn_exchange_unpack(ssn_sim* sim, const void* src_dev) {
  if (!sim || !src_dev) return fail(SSN_EINVAL, "null argument");
  return sim->exchange_copy(const_cast<void*>(src_dev), false);
}
int ssn_phase_async(ssn_sim* sim, int32_t phase, void* exchange_buf, void* hip_stream) {
  return sim ? sim->phase_async(phase, exchange_buf, (hipStream_t)hip_stream) : fail(SSN_EINVAL, "null simulator");
}
int ssn_phase_sync(ssn_sim* sim, void* hip_stream) { return sim ? sim->phase_sync((hipStream_t)hip_stream) : fail(SSN_EINVAL, "null simulator"); }
int ssn_get_kernel_times(ssn_sim* sim, ssn_kernel_time* out, int32_t capacity) {
  if (!sim || (!out && capacity > 0) || capacity < 0) return fail(SSN_EINVAL, "null argument");
  return sim->kernel_times(out, capacity);
}
int64_t ssn_n_steps(ssn_sim* sim) { return sim ? sim->n_steps() : -1; }
int ssn_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
const char* ssn_last_error(void) { return g_err.c_str(); }
const char* ssn_version(void) { return "libssn_hip 0.11 (gfx950, ABI 11)"; }

}  // extern "C"
