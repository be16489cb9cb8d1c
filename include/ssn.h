/* ssn.h - C ABI of libssn_hip.so: the MI355X (gfx950) step-loop backend for SSP-SLAM spiking networks.
 *
 * Drop-in boundary.  The reference has no FFI of its own: its hot path is the
 * Python call  `sim = nengo.Simulator(model); with sim: sim.run(T); sim.data[probe]`
 * (reference experiments/run_pathint.py:147-165,171-181; experiments/run_slam.py:198-235,250-268),
 * whose per-timestep arithmetic is executed by the third-party `nengo` / `nengo_ocl` simulators.
 * This library replaces that simulator core.  A thin ctypes wrapper (sspslam_amd/simulator.py)
 * exposes the same Simulator API on top of the entry points below; each entry point names the
 * Simulator member it serves.
 *
 * Model = one flat signal vector + parameter/state buffers + an ordered operator list (the frozen
 * "BuiltModel", produced on the host by sspslam_amd/builder.py).  All host arrays are float64 (or
 * int32 for index buffers), borrowed for the duration of the call only and converted to the
 * simulator's arithmetic type on upload.  The library owns all device memory.
 *
 * Every call returns SSN_OK (0) or a negative error code; ssn_last_error() gives the message
 * (thread-local).  One host thread drives a simulator; nothing calls back into the host during
 * ssn_run_steps.
 */
#ifndef SSN_H
#define SSN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSN_ABI_VERSION 11

enum ssn_status {
  SSN_OK = 0,
  SSN_EINVAL = -1,        /* bad argument / inconsistent model description        */
  SSN_EHIP = -2,          /* a HIP runtime call failed (message has the HIP error) */
  SSN_ERCCL = -3,         /* reserved                                             */
  SSN_ENOMEM = -4,        /* host or device allocation failed                     */
  SSN_EUNSUPPORTED = -5   /* operator shape outside what the kernels implement    */
};

enum ssn_dtype { SSN_F32 = 0, SSN_F64 = 1 };           /* arithmetic + state type of a simulator   */
enum ssn_buffer_kind { SSN_BUF_REAL = 0, SSN_BUF_I32 = 1, SSN_BUF_TAPS = 2 /* ssn_tap_desc records: ssn_model_desc.n_taps */,
                       SSN_BUF_DRIVES = 3 /* ssn_drive_desc records (ABI 10): found by kind, count = number of records */ };
enum ssn_neuron { SSN_LIF = 0, SSN_LIFRATE = 1, SSN_RELU = 2 };

/* Operator kinds; field use per kind is listed next to ssn_op_desc. */
enum ssn_op_kind {
  SSN_OP_FILL = 1, SSN_OP_TABLE = 2, SSN_OP_AXPY = 3, SSN_OP_MATVEC = 4, SSN_OP_LOWPASS = 5,
  SSN_OP_ENSARRAY = 6, SSN_OP_NEURONS = 7, SSN_OP_PES = 8, SSN_OP_VOJA = 9, SSN_OP_CLEANUP = 10,
  SSN_OP_GATE = 11, SSN_OP_LINCOMB = 12
};

typedef struct ssn_buffer_desc {
  const void* data;     /* float64 (SSN_BUF_REAL) or int32 (SSN_BUF_I32) host array, C order; ssn_tap_desc records (SSN_BUF_TAPS) */
  int64_t count;        /* number of elements (records)                                     */
  int32_t kind;         /* ssn_buffer_kind                                                  */
  int32_t reserved;
} ssn_buffer_desc;

/* One operator.  Offsets are element offsets into the signal vector; "buf" = index into buffers[].
 *  FILL     i0 dst  i1 len                                  f0 value
 *  TABLE    i0 dst  i1 width i2 table_id                                      (ssn_set_table)
 *  AXPY     i0 dst  i1 src   i2 len  i3 mode(0 inc,1 set)   f0 alpha
 *  MATVEC   i0 dst  i1 src   i2 rows i3 cols i4 W buf i5 mode i6 dft          W is rows x cols; dft != 0: W is
 *           the real-DFT map of a circular-convolution network (1-4 transform_in A / B / conj A / conj B, 5 transform_out,
 *           reference binding.py:23-74) - the f32 core may then run k_dft (mixed-radix FFT) instead of W
 *  LINCOMB  i0 dst  i1 len   i2 n_terms i3 src buf (int32 [n_terms]: signal offsets) i4 alpha buf (real [n_terms])
 *                                                           f0 self f1 const  dst=self*dst+(const+sum_k alpha_k*sig[src_k+i])
 *           (the folded linear glue between two big operators - chains of nengo Reset / ElementwiseInc / copy operators
 *           collapsed at build time; per-timestep core only)
 *  LOWPASS  i0 dst  i1 src   i2 len                         f0 a  f1 gain     dst=a*dst+(1-a)*gain*src
 *  ENSARRAY i0 x    i1 K i2 n i3 din i4 dout i5 enc buf [K][din][n] i6 bias buf [K][n]
 *           i7 dec buf [K][dout][n] i8 dst_idx buf (int32 [K][dout]) i9 V buf i10 R buf
 *           i11 neuron                                      f0 tau_rc f1 tau_ref f2 min_voltage
 *           (all twelve i[] slots are taken: the neuron taps of an array travel as ssn_tap_desc records, ssn_model_desc.n_taps,
 *            its neuron-input drive columns as ssn_drive_desc records, SSN_BUF_DRIVES)
 *  NEURONS  i0 J    i1 out   i2 n i3 V buf i4 R buf i5 neuron  f0 tau_rc f1 tau_ref f2 min_voltage f3 amp
 *  PES      i0 W buf i1 rows i2 cols i3 err i4 act          f0 kappa          W += kappa*outer(err,act)
 *  VOJA     i0 E buf i1 rows i2 cols i3 spk i4 key i5 learn i6 scale buf  f0 lr*dt
 *  CLEANUP  i0 dst  i1 src   i2 rows i3 cols i4 table buf                     dst = T[argmax(T@src)]
 *           optional factor tables of a sample grid (i5 != 0; buffer ids + 1): i5 dft buf (2K x cols: Re / Im rows of the
 *           half spectrum), i6 lhs buf (i8 x 2K), i7 rhs buf (i9 x 2K), i8 * i9 = rows, i10 = 2K, (Re, Im) interleaved, with
 *           T[a * i9 + r] . x = sum_k Re(conj(X_k) lhs[a, k] rhs[r, k]) - the f32 core then forms the similarities of a
 *           large table (>= 64 MB) as one MFMA product instead of a pass over the table (reference slam.py:209-215)
 *  GATE     i0 dst  i1 src   i2 d                           f0 thres f1 rate  (reference slam.py:233-237)
 * level: scheduling round from the host builder; vector ops of equal level touch disjoint data. */
typedef struct ssn_op_desc {
  int32_t kind;
  int32_t level;
  int32_t stage;        /* 0 pre, 1 core (stepped one timestep at a time), 2 post; pre/post run time-batched  */
  int32_t border;       /* position in the time-batched order of its stage (pre/post), else -1              */
  int32_t src_prev;     /* batched: source operand is a synapse state read before its update (previous row) */
  int32_t phase;        /* neuron-sharded models: 0 = before the per-timestep exchange, 1 = after it (the updates)  */
  int64_t i[12];
  double f[4];
} ssn_op_desc;

typedef struct ssn_probe_desc {
  int64_t src;          /* signal offset  */
  int64_t width;
  int64_t every;        /* sample when (step % every) == 0, steps counted from 1 */
  int64_t stage;        /* 1: sampled by the core every step; 0/2: sampled by a time-batched stage */
} ssn_probe_desc;

typedef struct ssn_range { int64_t lo, hi; } ssn_range;   /* signal range [lo, hi) */

/* Neuron tap of an ENSARRAY operator (ABI 9): after the neuron step of every timestep
 *   sig[dst + j] = amp * a[k][first + j],  j = 0 .. count - 1
 * with a the unit-amplitude neuron output of ensemble k (spike 0 / 1, or the rate): what Probe(member.neurons[first:first+count])
 * samples.  At most one tap per ensemble; the tap signals overlap neither each other nor the operator's decoded rows.
 * The records travel as the LAST entry of ssn_model_desc.buffers, kind SSN_BUF_TAPS, count = ssn_model_desc.n_taps (the
 * descriptor keeps its size and field offsets: n_taps took its spare word, and no operator refers to that buffer). */
typedef struct ssn_tap_desc {
  int32_t op;           /* index into ops[]: an SSN_OP_ENSARRAY of the per-timestep core */
  int32_t k;            /* ensemble of that array, 0 .. K - 1 */
  int64_t first, count; /* neurons [first, first + count) of it, inside 0 .. n */
  int64_t dst;          /* signal offset of the tap's first element */
  double amp;           /* amplitude / dt for spiking LIF, amplitude for the rate neurons */
} ssn_tap_desc;

/* Direct neuron input of an ENSARRAY operator (ABI 10): m drive columns per ensemble,
 *   J[k][i] = (bias[k][i] + enc[k][.][i] . x[k]) + sum_j w[k][j][i] * sig[src[k][j]],  j = 0 .. m - 1 in order
 * src[k][j] = -1 marks an unused slot (its weights are ignored: the term is 0).  The sources are read when the inputs x are.
 * The records travel as one buffer of kind SSN_BUF_DRIVES, found by its kind (at most one; count = number of records; no
 * operator refers to it; the taps buffer, if any, stays the last entry).  A driven array is stepped by the per-timestep array
 * kernel on a launch of its own; SSN_PLAN_SPLIT_BLOCK is refused with drives as it is with taps. */
typedef struct ssn_drive_desc {
  int32_t op;           /* index into ops[]: an SSN_OP_ENSARRAY of the per-timestep core; one record per operator at most */
  int32_t m;            /* columns per ensemble, 1 .. 4 */
  int32_t w_buf;        /* SSN_BUF_REAL [K][m][n] */
  int32_t src_buf;      /* SSN_BUF_I32 [K][m]: signal offset of each column's scalar, or -1 */
} ssn_drive_desc;

/* Plan switches: the bits of ssn_model_desc.flags.  Debug / A-B switches, default 0; tests check that every alternative
 * plan gives the same results.  ssn_create refuses a value with any other bit set.
 * (Round 1's opt-in experiments 32, 64, 2048, 16384, 32768 the multi-stream step graph 256 and the program-planner
 *  switches 65536, 131072, 1048576 of the round-1 plan - all measured slower - were removed.) */
enum ssn_plan_flag {
  /* no fused recurrent-array core (generic programs) */
  SSN_PLAN_NO_FUSED_CORE = 1,
  /* no LIF fast path (unpacked state, dense row-major decoders) */
  SSN_PLAN_NO_LIF_FAST = 2,
  /* LIF fast path with dense decoders (no spike-sparse gather) */
  SSN_PLAN_DENSE_DECODERS = 4,
  /* dense decoder products for dense ensembles (no k_spmv_partial) */
  SSN_PLAN_NO_SPMV = 8,
  /* fused recurrent-array core always with a separate finish kernel
   * (default: finish deferred into the next step's prologue, 1 launch per step) */
  SSN_PLAN_SEPARATE_FINISH = 16,
  /* no whole-block kernel for a recurrent array of independent ensembles (k_ens_block): step it once per timestep
   * (k_ensarray) instead */
  SSN_PLAN_NO_BLOCK_KERNEL = 128,
  /* no FFT kernel for DFT-structured matvecs (always multiply by the matrix) */
  SSN_PLAN_NO_FFT = 512,
  /* k_spmv_partial rebuilds the spike list itself (no segmented list from k_neurons) */
  SSN_PLAN_SPMV_OWN_LIST = 1024,
  /* one launch per operator (adjacent independent operators of one kind are not batched); only acts together with
   * SSN_PLAN_NO_ROUNDS */
  SSN_PLAN_NO_ITEM_BATCH = 4096,
  /* ensemble arrays always leave partial sums for a finish operator (no direct write when one workgroup covers an
   * ensemble) */
  SSN_PLAN_ENS_PARTIALS = 8192,
  /* one launch per element-wise operator of the time-batched stages (no batching) */
  SSN_PLAN_NO_STAGE_BATCH = 262144,
  /* clean-up similarities always from the pass over the table (no factored grid) */
  SSN_PLAN_NO_FACTORED_GRID = 524288,
  /* no rounds: one launch per big operator and one k_program launch per run of small ones (the round-1 plan).
   * Default: every operator takes the earliest round its data hazards allow and a round is ONE heterogeneous grid
   * (k_round) */
  SSN_PLAN_NO_ROUNDS = 2097152,
  /* ensemble arrays are launched on their own, not as bodies of the round's grid */
  SSN_PLAN_ENS_OWN_LAUNCH = 4194304,
  /* the rounds of one timestep at a time (default: the steps_per_graph timesteps of a step graph are
   * software-pipelined - an operator of step s + 1 may share a round with operators of step s) */
  SSN_PLAN_NO_PIPELINE = 8388608,
  /* heavy operators stay whole (default: the pipelined plan may run the blocks of a bandwidth-bound operator in pieces
   * over the rounds of its slack window) */
  SSN_PLAN_NO_BALANCE = 16777216,
  /* merged element-wise operators stay whole (default: cut at the range endpoints of the other operators, so that each
   * piece has its own hazards) */
  SSN_PLAN_NO_CUTS = 33554432,
  /* no chains (default: an element-wise micro-operator whose only hazards inside a round are on identical element
   * ranges joins that round and runs behind its predecessor in the same block) */
  SSN_PLAN_NO_CHAINS = 134217728,
  /* k_dft also for chirp-z (Bluestein) transforms of 2048 points and more (default: their dense matrix - one workgroup
   * needs 40 us for such a transform) */
  SSN_PLAN_BLUESTEIN_FFT = 268435456,
  /* the four-step FFT on the matrix cores (two small dense DFTs as f32 MFMA products around a twiddle multiply, round 3;
   * any factorisation, primes up to 192 as one dense DFT) instead of the Stockham passes (generic radix-r butterflies
   * through LDS).  Correct for every length of the tests, but measured no faster (its operand loads are
   * latency-bound): opt-in */
  SSN_PLAN_FOUR_STEP_FFT = 536870912,
  /* split ensembles in the whole-block kernel (f32, at most 4 decoded rows): an array with fewer ensembles than the GPU
   * has CUs (a 4- or 8-GPU shard of config 2) is stepped by 2 or 4 member workgroups per ensemble that exchange their
   * partial sums every timestep; needs every workgroup of the launch resident at once, i.e. the GPU for this process
   * alone.  Not available for an array with neuron taps or drive columns (ssn_create: SSN_EUNSUPPORTED) */
  SSN_PLAN_SPLIT_BLOCK = 1073741824
};
/* every bit that has a name */
#define SSN_PLAN_ALL_FLAGS                                                                                                   \
  (SSN_PLAN_NO_FUSED_CORE | SSN_PLAN_NO_LIF_FAST | SSN_PLAN_DENSE_DECODERS | SSN_PLAN_NO_SPMV | SSN_PLAN_SEPARATE_FINISH |   \
   SSN_PLAN_NO_BLOCK_KERNEL | SSN_PLAN_NO_FFT | SSN_PLAN_SPMV_OWN_LIST | SSN_PLAN_NO_ITEM_BATCH | SSN_PLAN_ENS_PARTIALS |    \
   SSN_PLAN_NO_STAGE_BATCH | SSN_PLAN_NO_FACTORED_GRID | SSN_PLAN_NO_ROUNDS | SSN_PLAN_ENS_OWN_LAUNCH |                      \
   SSN_PLAN_NO_PIPELINE | SSN_PLAN_NO_BALANCE | SSN_PLAN_NO_CUTS | SSN_PLAN_NO_CHAINS | SSN_PLAN_BLUESTEIN_FFT |             \
   SSN_PLAN_FOUR_STEP_FFT | SSN_PLAN_SPLIT_BLOCK)

typedef struct ssn_model_desc {
  int32_t abi_version;  /* SSN_ABI_VERSION */
  int32_t dtype;        /* ssn_dtype       */
  int32_t device;       /* HIP device index */
  int32_t n_tables;
  double dt;
  int64_t n_signals;
  const double* signal_init;          /* n_signals values */
  int32_t n_buffers;
  int32_t n_ops;
  int32_t n_probes;
  int32_t steps_per_graph;            /* timesteps captured per hipGraph (at most 128); 0 = library default (64 where blocks hold whole graphs, else 16), 1 = no graph */
  const ssn_buffer_desc* buffers;
  const ssn_op_desc* ops;
  const ssn_probe_desc* probes;
  /* stage boundaries (host builder, stages.py): signals the pre stage hands to the core at the start of
   * each timestep, and signals the core hands to the post stage at the end of each timestep */
  int32_t n_pre_to_core;
  int32_t n_core_to_post;
  const ssn_range* pre_to_core;
  const ssn_range* core_to_post;
  /* Neuron-sharded model (one rank of a SLAMNetwork split over several GPUs): the partial sums in these signal
   * ranges are completed by an all-reduce between the two phases of every timestep.  The library does not communicate: the
   * caller steps with ssn_run_phase(0), exchanges (ssn_exchange_pack -> all-reduce -> ssn_exchange_unpack), ssn_run_phase(1). */
  int32_t n_exchange;
  int32_t n_taps;                     /* neuron taps of the ensemble arrays (ABI 9; 0: none): buffers[n_buffers - 1] then holds n_taps ssn_tap_desc records */
  const ssn_range* exchange;
  int32_t block_steps;                /* timesteps per time-batched block; 0 = library default (1024, or 256 for very wide models) */
  int32_t flags;                      /* plan switches: an OR of ssn_plan_flag values (default 0) */
} ssn_model_desc;

typedef struct ssn_counters {
  int64_t n_steps;                  /* steps executed since create/reset                          */
  int64_t launches_per_step;        /* kernel launches in one timestep                            */
  int64_t dominant_launches;        /* timed launches of the dominant (ensemble-array) kernel      */
  double dominant_ms_total;         /* sum of their durations, HIP events on the launching stream */
  double dominant_bytes_per_launch; /* algorithmic bytes of one such launch           */
  int64_t dominant_units_per_launch;/* neuron-steps per launch                                    */
  double last_run_ms;               /* device time of the last ssn_run_steps (events)             */
  int64_t device_bytes;             /* device memory held by this simulator                       */
  /* whole-block kernel (k_ens_block) variant the planner picked; all 0 when the core is stepped per timestep */
  int32_t block_tpb;                /* workgroup size the variant is compiled for                  */
  int32_t block_npt;                /* neurons per thread                                         */
  int32_t block_enc_lds;            /* 1: encoders live in LDS, 0: in registers                   */
  int32_t block_threads;            /* threads actually launched per workgroup                    */
  int32_t fft_transforms;           /* DFT-structured matvecs of a timestep that run as k_dft (FFT) instead of the matrix */
  int32_t fft_bluestein;            /* ... of which through Bluestein's convolution (a prime factor > 32)           */
  int32_t block_members;            /* member workgroups per ensemble of the whole-block kernel (SSN_PLAN_SPLIT_BLOCK; 1 = not split, 0 = no block kernel) */
  int32_t batch_products_skipped; /* time-batched products not multiplied out because their whole input was zero over the block (cumulative) */
  /* whole-block kernel (f32): (wave, round) slots stepped since create / reset, and how many of them were silent - no neuron of the
   * slot spiked in the timestep, so the spike-time arithmetic and the decode were left out (ABI 7; the VALU roofline of bench.py
   * prices the two paths with these) */
  int64_t block_slots;
  int64_t block_slots_silent;
  /* round plan (ABI 8) */
  int32_t fused_populations;        /* dense populations whose neuron update runs in the epilogue of their encoder product      */
  int32_t serial_chains;            /* serial chains of single-workgroup operators in one timestep's rounds (the eager plan)    */
} ssn_counters;

/* Per-kernel device time of the generic (one launch per operator) plan, collected by ssn_run_steps(profile = 2):
 * every launch of the timed timesteps is bracketed with HIP events on the simulator's stream. */
typedef struct ssn_kernel_time {
  char name[32];                    /* kernel of the plan item: "k_program", "k_matvec", "k_ensarray", ... */
  int64_t launches;
  double ms_total;
} ssn_kernel_time;

typedef struct ssn_sim ssn_sim;

/* Simulator(network): upload the built model, plan kernels, capture the step graph. */
int ssn_create(const ssn_model_desc* desc, ssn_sim** out);
/* Simulator.close() / __exit__ */
void ssn_destroy(ssn_sim* sim);
/* Simulator.reset(): restore initial signals, neuron state and learned buffers; step = 0. */
int ssn_reset(ssn_sim* sim);

/* Pre-tabulated output of a t-only Node (the host evaluates the user's closure once per step of
 * the coming run): rows[n_rows][width] unique rows, idx[n_idx] row per step (-1 = zeros) for steps
 * first_step .. first_step+n_idx-1 (0-based).  Serves Node(lambda t: ...) at run_pathint.py:134-136. */
int ssn_set_table(ssn_sim* sim, int32_t table_id, const double* rows, int64_t n_rows, int64_t width,
                  const int32_t* idx, int64_t n_idx, int64_t first_step);
/* Same, rows already on the device in the simulator's dtype (multi-GPU exchange path). */
int ssn_set_table_device(ssn_sim* sim, int32_t table_id, const void* rows_dev, int64_t n_rows,
                         int64_t width, const int32_t* idx, int64_t n_idx, int64_t first_step);

/* The same in two halves for chunked runs (Simulator.run(T) over many chunks: the node closures of chunk k + 1 are evaluated
 * while the device steps chunk k, reference run_pathint.py:160-165 times the whole of it): ssn_stage_table takes rows ALREADY in
 * the simulator's dtype (float for SSN_F32, double for SSN_F64) and copies them by DMA into a second set of device buffers - it
 * may be called from another host thread while ssn_run_steps is in flight; ssn_commit_tables, called between two runs, makes
 * every staged table the current one.  (ABI 7) */
int ssn_stage_table(ssn_sim* sim, int32_t table_id, const void* rows_typed, int64_t n_rows, int64_t width,
                    const int32_t* idx, int64_t n_idx, int64_t first_step);
int ssn_commit_tables(ssn_sim* sim);

/* Make room for the probe samples of the next n_steps (drops samples already read). */
int ssn_reserve_probes(ssn_sim* sim, int64_t n_steps);
/* Simulator.run_steps(n): blocking. profile = 1 times every dominant-kernel launch with events; profile = 2 times
 * every launch of the per-timestep plan (eager launches instead of graph replay) for ssn_get_kernel_times. */
int ssn_run_steps(ssn_sim* sim, int64_t n, int32_t profile);
/* Simulator.data[probe]: samples [first, first+count) of the current reservation -> dst[count][width]. */
int ssn_read_probe(ssn_sim* sim, int32_t probe_id, double* dst, int64_t first, int64_t count);
/* Same into device memory (simulator dtype), no host round trip. */
int ssn_read_probe_device(ssn_sim* sim, int32_t probe_id, void* dst_dev, int64_t first, int64_t count);
int64_t ssn_probe_count(ssn_sim* sim, int32_t probe_id);

/* Signals and buffers (learned weights, encoders, neuron state): checkpointing, tests, weight probes. */
int ssn_read_signal(ssn_sim* sim, int64_t off, int64_t count, double* dst);
int ssn_write_signal(ssn_sim* sim, int64_t off, int64_t count, const double* src);
int ssn_read_buffer(ssn_sim* sim, int32_t buffer_id, double* dst, int64_t count);
int ssn_write_buffer(ssn_sim* sim, int32_t buffer_id, const double* src, int64_t count);

/* Neuron-sharded models: one half of a timestep (phase 0: everything up to the exchange; phase 1: the updates, probe
 * sampling, step counter; phase 2 = phase 1 followed by phase 0 of the next timestep in one launch, for the inside of a
 * run: 0, x, 2, x, 2, ..., x, 1 with x the caller's exchange).  Blocking.  ssn_run_steps refuses such models. */
int ssn_run_phase(ssn_sim* sim, int32_t phase);
/* Pipelined over the exchange (ABI 8): C = ssn_cycle_steps() timesteps planned together as C + 1 launch segments, the exchange
 * of timestep k between segments k and k + 1 - what does not hang on that exchange (the head of timestep k + 1) shares rounds
 * with what does.  phase = 3 (ssn_run_phase and ssn_phase_async alike) runs the next segment; a cycle is
 *   3, x, 3, x, ..., x, 3   (C + 1 segments, C exchanges x)
 * it starts at a timestep boundary, and phases 0 / 1 / 2 are refused until its last segment has run (they serve the timesteps that
 * do not fill a cycle).  0: the model has no such plan (not neuron-sharded, or planned with flag 8388608 / SSN_CYCLE_STEPS=0). */
int64_t ssn_cycle_steps(ssn_sim* sim);
/* Elements of the exchange (sum of the range lengths); copy them to / from one contiguous device buffer of the simulator's dtype. */
int64_t ssn_exchange_size(ssn_sim* sim);
int ssn_exchange_pack(ssn_sim* sim, void* dst_dev);
int ssn_exchange_unpack(ssn_sim* sim, const void* src_dev);

/* Stream-ordered stepping of a neuron-sharded model: no host synchronisation per timestep (SURVEY 8b "no callbacks into Python
 * from the step loop", 8e; the loop it serves closes every timestep: reference networks/slam.py:259,306-307).  Enqueues, as ONE
 * graph launch on `hip_stream` (a hipStream_t of the caller - the stream its collective is ordered on, e.g. the current stream of
 * torch.distributed's RCCL backend; NULL = the simulator's own stream), and returns without waiting:
 *   [phase 1 / 2: exchange_buf (the all-reduced sums) -> the exchange ranges]  the phase's kernels
 *   [phase 0 / 2: the exchange ranges (this rank's partial sums) -> exchange_buf]
 * exchange_buf: device buffer of ssn_exchange_size() elements of the simulator's dtype, the same pointer throughout a run (it is
 * captured into the graphs); NULL when the caller does not exchange (a single rank).  A run is
 *   ssn_phase_async(0), [collective on hip_stream], ssn_phase_async(2), [collective], ..., ssn_phase_async(1), ssn_phase_sync.
 * phase = -1 only builds the graphs for exchange_buf (otherwise built by the first call of a run) and launches nothing;
 * phase = 3: the next segment of a pipelined cycle (ssn_cycle_steps above), [unpack] / [pack] around it as for phases 2 / 0. */
int ssn_phase_async(ssn_sim* sim, int32_t phase, void* exchange_buf, void* hip_stream);
/* Waits for everything ssn_phase_async enqueued on that stream; checks the device step counter and the probe-overflow flag. */
int ssn_phase_sync(ssn_sim* sim, void* hip_stream);

/* Measurement aid for the roofline of the VALU-bound whole-block kernel (bench.py; not on the step path): `iters` x 64 independent
 * wave64 instructions of one kind per wave, one workgroup of 256 x waves_per_simd threads on every CU; reports the nanoseconds of
 * SIMD time per wave instruction from the launch's HIP-event time (and the shader clock during the launch, s_memtime ticks per
 * 100 MHz s_memrealtime tick).  csrc/ssn_probe.hip. */
enum ssn_probe_kind {
  SSN_PROBE_PK_FMA = 0, SSN_PROBE_PK_MUL = 1, SSN_PROBE_PK_ADD = 2,   /* v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32            */
  SSN_PROBE_TRANS = 3,                                                /* v_rcp_f32 (v_log_f32 issues at the same rate)        */
  SSN_PROBE_FMA = 4, SSN_PROBE_ADD = 5,                               /* v_fma_f32; v_add_f32 (v_mul_f32, v_sub_f32)          */
  SSN_PROBE_DPP = 6, SSN_PROBE_MOV = 7, SSN_PROBE_READLANE = 8,       /* v_add_f32_dpp; v_mov_b32; v_readlane_b32             */
  SSN_PROBE_CNDMASK = 9, SSN_PROBE_OTHER = 10,                        /* v_cndmask_b32 (vcc); v_max_i32 (every other VALU op) */
  SSN_PROBE_N_KINDS = 11
};
int ssn_probe_issue_rate(int32_t device, int32_t kind, int32_t waves_per_simd, int32_t iters,
                         double* ns_per_wave_instruction, double* shader_mhz);

/* Grid decoding of SSP trajectories (ABI 11; csrc/ssn_decode.hip): SSPSpace.decode(rows, 'from-set', 'grid', n) on the device,
 * reference run_pathint.py:171-179, run_slam.py:242-268.  A decoder holds a sample table (n_samples x width host doubles, C order,
 * converted to `dtype` and uploaded once) and a scratch area whose size is fixed at creation (0 = 64 MB; at least one 128-row tile:
 * ssn_decoder_info.min_scratch_bytes); it is independent of ssn_sim and may outlive or precede any simulator.  Every input row is
 * scaled as the host scales it (divided by its norm when the norm is >= 1e-6, left as it is otherwise) and
 *   best[t] = argmax_j sum_k row_t[k] table[j][k]      (lowest j on ties; sims[t], when not NULL, is that largest similarity)
 * f32 runs on the f32-input matrix cores (each similarity an exact k-ordered fmaf chain), f64 is the parity mode.  The n_rows x
 * n_samples similarity matrix is never stored; the results do not depend on the scratch size and are the same from run to run.
 * Non-finite input is out of contract: best[] stays inside [0, n_samples).  best / sims are host arrays, filled when the call returns.
 * SSN_EINVAL: null handle or argument, width 0, n_samples 0 or above 2^31 - 1, scratch too small for one tile;
 * SSN_EHIP "no HIP device available (there is no CPU fallback)" without a GPU; n_rows == 0 succeeds and writes nothing. */
typedef struct ssn_decoder ssn_decoder;
typedef struct ssn_decoder_info {
  int64_t row_chunk;          /* rows per chunk (whole tiles) for the n_rows asked about                         */
  int64_t n_chunks;
  int64_t n_strips;           /* column strips: workgroups per row tile, partials per row                        */
  int64_t tiles_per_strip;    /* column tiles a workgroup walks                                                  */
  int64_t tile;               /* rows and columns of a tile (128)                                                */
  int64_t scratch_bytes;
  int64_t min_scratch_bytes;  /* one row tile with one strip                                                     */
  int64_t slot_bytes;         /* what one more strip of a row tile costs                                         */
  int64_t padded_width;
  int64_t last_launches;      /* kernel launches of the last ssn_decoder_rows* call                              */
  double last_kernel_ms;      /* their device time (HIP events around the kernels of every chunk, copies outside) */
} ssn_decoder_info;
int ssn_decoder_create(int32_t dtype, int32_t device, const double* table, int64_t n_samples, int64_t width,
                       int64_t scratch_bytes /* 0 = default */, ssn_decoder** out);
void ssn_decoder_destroy(ssn_decoder* dec);
int ssn_decoder_rows(ssn_decoder* dec, const double* rows, int64_t n_rows, int32_t* best, double* sims /* may be NULL */);
/* rows already on the decoder's device: rows_dtype SSN_F32 / SSN_F64, leading dimension ld >= width (elements) */
int ssn_decoder_rows_device(ssn_decoder* dec, const void* rows_dev, int32_t rows_dtype, int64_t ld, int64_t n_rows,
                            int32_t* best, double* sims);
/* How a call with n_rows rows is cut into row chunks and column strips, and the device time of the last call. */
int ssn_decoder_get_info(ssn_decoder* dec, int64_t n_rows, ssn_decoder_info* out);
/* Measurement aid (tools/bench_decode.py): the same answer from the composition the fused kernel replaces - k_gemm_nt_mfma_f32 into
 * an n_rows x n_samples buffer (at most 2 GB, allocated for the call), then k_argmax_partial; f32 decoders, one row chunk. */
int ssn_decoder_rows_composed(ssn_decoder* dec, const double* rows, int64_t n_rows, int32_t* best);

/* Sub-grid refinement of the grid decode (additive to ABI 11; the rule is written out at k_decode_refine in csrc/ssn_decode.hip and
 * in DESIGN.md 3.12): from the grid argmax x0 of a row, `iterations` safeguarded Newton steps on
 *   f(x) = sum_k c_k cos(M_k . x) + s_k sin(M_k . x),   c_k + i s_k = w_k fft(row / |row|)_k,
 * clipped to the box [max(lo, x0 - pitch), min(hi, x0 + pitch)].  ssn_decoder_set_refine uploads the tables (all host doubles, C
 * order): dft (2K x width: row 2k = Re, row 2k + 1 = Im of exp(-2 pi i k c / width), unweighted - w is folded in here), M (K x dim,
 * phase_matrix / length_scale of the K bins used), w (K), points (n_samples x dim: the decoder's sample points), lo / hi / pitch
 * (dim each).  dim is 1, 2 or 3.  It may be called again to replace the tables.
 * ssn_decoder_refine_rows* then fill host arrays: x (n_rows x dim), best (the grid index), f (f at x) and status (bit 1: x on a box
 * face, 2: Hessian not negative definite at x, 4: last step above 1e-6 pitch on some axis); best, f and status may be NULL.
 * iterations == 0 returns points[best] exactly.  The results do not depend on the scratch size and are the same from run to run.
 * SSN_EINVAL: null handle or argument, dim outside 1..3, negative iterations, refinement before ssn_decoder_set_refine;
 * n_rows == 0 succeeds and writes nothing. */
int ssn_decoder_set_refine(ssn_decoder* dec, const double* dft, int64_t K, const double* M, const double* w, int32_t dim,
                           const double* points, const double* lo, const double* hi, const double* pitch);
int ssn_decoder_refine_rows(ssn_decoder* dec, const double* rows, int64_t n_rows, int32_t iterations, double* x, int32_t* best,
                            double* f, int32_t* status);
int ssn_decoder_refine_rows_device(ssn_decoder* dec, const void* rows_dev, int32_t rows_dtype, int64_t ld, int64_t n_rows,
                                   int32_t iterations, double* x, int32_t* best, double* f, int32_t* status);

/* Similarity maps (additive to ABI 11; k_decode_map in csrc/ssn_decode.hip): the n_rows x n_samples similarities
 * the decode compares, kept:  out[t * out_ld + j] = (sum_k row_t[k] table[j][k]) ^ (1 or 2).  flags: SSN_MAP_NORMALIZE scales every
 * row as the decode does (otherwise the rows are used raw), SSN_MAP_SQUARE stores s * s (one multiply in the decoder's dtype).
 * rows: n_rows x width host doubles, dense (rows_on_device == 0; rows_dtype and rows_ld are ignored), or rows on the decoder's
 * device of rows_dtype SSN_F32 / SSN_F64 with leading dimension rows_ld >= width (elements).  out: host memory (out_on_device == 0)
 * or memory on the decoder's device, of out_dtype = the decoder's dtype, or SSN_F64 from an f32 decoder (exact widening; SSN_F32
 * from an f64 decoder is not offered), with leading dimension out_ld >= n_samples (elements).  Only out[t][j], t < n_rows,
 * j < n_samples, is written - padding up to out_ld is left alone - and the map is complete when the call returns.  Every stored
 * value is the accumulator ssn_decoder_rows compares (with SSN_MAP_NORMALIZE), so the argmax of a row, lowest index on ties, is
 * best[t]; the bits do not depend on the scratch or stage size, on where rows and output live, or on the run.
 * A device output is written in place.  A host output goes through a device stage and pinned host memory of the same size, made on
 * first use: ssn_decoder_set_map_stage sets that size (0 = the default: 64 MB, or one 128-row tile of doubles, 1024 n_samples
 * bytes, when that is more); rows per chunk are the whole tiles that fit both the row scratch and the stage, never n_rows x
 * n_samples.  The copy back of a chunk is not overlapped with the kernels of the next.  ssn_decoder_get_info reports
 * last_launches / last_kernel_ms of a map call (prepare + k_decode_map of every chunk) as of a decode call.
 * SSN_EINVAL: null handle or argument, unknown flags or dtype, rows_ld below the width, out_ld below n_samples, an out_dtype
 * narrower than the decoder's, a stage below one tile (128 n_samples elements of the decoder's dtype in ssn_decoder_set_map_stage, of
 * out_dtype in ssn_decoder_map); n_rows == 0 succeeds and writes nothing. */
enum { SSN_MAP_NORMALIZE = 1, SSN_MAP_SQUARE = 2 };
int ssn_decoder_map(ssn_decoder* dec, const void* rows, int32_t rows_on_device, int32_t rows_dtype, int64_t rows_ld, int64_t n_rows,
                    int32_t flags, void* out, int32_t out_on_device, int32_t out_dtype, int64_t out_ld);
int ssn_decoder_set_map_stage(ssn_decoder* dec, int64_t bytes /* 0 = default */);

/* SSP encoding of points on the device (additive to ABI 11; csrc/ssn_encode.hip): SSPSpace.encode as a phase
 * kernel and one product.  With K bins, M (K x dim: phase_matrix / length_scale of the bins used) and w (K) - what
 * SSPSpace.refine_tables() returns, host doubles, C order - and th_k = M_k . x,
 *   encode(x)[c] = sum_{k<K} w_k ( cos th_k cos(2 pi k c / d) - sin th_k sin(2 pi k c / d) ),   c = 0 .. d - 1.
 * th (an fma chain in axis order) and its sincos are float64 in both dtypes; the product is the k-ordered fmaf chain on the f32 matrix
 * cores (SSN_F32) or an ordered float64 fma chain (SSN_F64, the parity mode).  An encoder has a stream and a scratch area of its own
 * (0 = 64 MB; at least ssn_encoder_info.min_scratch_bytes, one 64-point tile) and is independent of ssn_sim.  Points are cut into
 * chunks that fit the scratch area; the results do not depend on its size, are the same for host and device points of the same
 * values and the same from run to run.
 * ssn_encoder_encode: n x dim host doubles (dense) -> n x d host doubles (the encoder's dtype widened).
 * ssn_encoder_encode_device: points on the host (points_on_device == 0) or on the encoder's device, points_dtype SSN_F32 / SSN_F64,
 * leading dimension points_ld >= dim (elements) -> a device buffer of the encoder's dtype with leading dimension out_ld >= d, complete
 * when the call returns.
 * SSN_EINVAL: null handle or argument, dim < 1, K < 1 or above d, d outside 1 .. 2^20, a leading dimension below the width, scratch
 * too small; SSN_EHIP "no HIP device available (there is no CPU fallback)" without a GPU; n == 0 succeeds and writes nothing. */
typedef struct ssn_encoder ssn_encoder;
typedef struct ssn_encoder_info {
  int64_t row_chunk;          /* points per chunk (whole tiles)                                                  */
  int64_t n_chunks;           /* for the n asked about                                                           */
  int64_t tile;               /* points per tile (64)                                                            */
  int64_t scratch_bytes;
  int64_t min_scratch_bytes;  /* one tile                                                                        */
  int64_t padded_2k;          /* columns of P and B: 2K padded to a multiple of 32                               */
  int64_t last_launches;      /* kernel launches of the last encode call                                         */
  double last_kernel_ms;      /* their device time (HIP events around the kernels of every chunk, copies outside) */
  double last_phase_ms;       /* of which k_encode_phase                                                         */
  double last_product_ms;     /* and the product (in f32 with the widening of a host-output call)                */
} ssn_encoder_info;
int ssn_encoder_create(int32_t dtype, int32_t device, int64_t d, int64_t K, int32_t dim, const double* M, const double* w,
                       int64_t scratch_bytes /* 0 = default */, ssn_encoder** out);
void ssn_encoder_destroy(ssn_encoder* enc);
int ssn_encoder_encode(ssn_encoder* enc, const double* points, int64_t n, double* out);
int ssn_encoder_encode_device(ssn_encoder* enc, const void* points, int32_t points_on_device, int32_t points_dtype, int64_t points_ld,
                              int64_t n, void* out_dev, int64_t out_ld);
int ssn_encoder_get_info(ssn_encoder* enc, int64_t n, ssn_encoder_info* out);
/* Region SSPs (additive to ABI 11): the SSP of an axis-aligned box in closed form.  A box row is lo_0, hi_0, lo_1,
 * hi_1, ... (2 dim values, the layout of domain_bounds).  With centre c, side lengths L and th_k = M_k . c, bin k of the box is
 * encode(c)'s bin times a real amplitude A_k, so a region is the same product on [A cos th, A sin th]:
 *   samples == NULL, mean == 0   the integral of encode over the box:  A_k = prod_a L_a sinc(M_ka L_a / 2),  sinc(y) = sin(y) / y
 *   samples == NULL, mean != 0   its mean (no L_a): a zero-width axis contributes 1, a zero-width box is encode(c) bit for bit
 *   samples (dim counts >= 2)    the sum of encode over the linspace mesh of samples[a] points per axis, both ends included:
 *                                A_k = prod_a sin(n_a y_a) / sin(y_a),  y_a = M_ka L_a / (2 (n_a - 1))
 * th, the amplitude and the sincos are float64 in both dtypes, the removable singularities (y = 0, which bin 0 of every box hits, and
 * y_a at a multiple of pi) go to their series below fixed thresholds; the product, the chunks and the determinism are those of the point
 * calls.  The box calls stage 2 dim doubles per row, so they need min_scratch_bytes + 64 * 8 * dim bytes of scratch.
 * ssn_encoder_encode_boxes: n x 2 dim host doubles (dense) -> n x d host doubles.
 * ssn_encoder_encode_boxes_device: boxes on the host or on the encoder's device, boxes_dtype SSN_F32 / SSN_F64, leading dimension
 * boxes_ld >= 2 dim -> a device buffer of the encoder's dtype with leading dimension out_ld >= d; normalize != 0 divides every row by
 * max(its norm, 1e-8) on the device (the sum of squares in float64, in a fixed order).
 * SSN_EINVAL beyond the point calls': "hi < lo" for a box with a negative side, "below 2" for a mesh count under 2, "mean given
 * together with samples", "too small for one 64-box tile" with the bytes needed. */
int ssn_encoder_encode_boxes(ssn_encoder* enc, const double* boxes, int64_t n, const int32_t* samples /* NULL: no mesh */, int32_t mean,
                             double* out);
int ssn_encoder_encode_boxes_device(ssn_encoder* enc, const void* boxes, int32_t boxes_on_device, int32_t boxes_dtype, int64_t boxes_ld,
                                    int64_t n, const int32_t* samples /* NULL: no mesh */, int32_t mean, int32_t normalize, void* out_dev,
                                    int64_t out_ld);
/* A decoder whose table is made on the device: the n_samples x dim sample points (host doubles) are encoded by a float64 encoder
 * (d = width, K, dim, M, w as above; enc_scratch_bytes its scratch area, 0 = default) chunk by chunk, each chunk written straight
 * into the decoder's padded table in the decoder's dtype.  The table never exists on the host; device memory peaks at the table
 * plus the two scratch areas.  The decoder is in every other respect the one ssn_decoder_create makes. */
int ssn_decoder_create_from_points(int32_t dtype, int32_t device, const double* points, int64_t n_samples, int64_t width, int64_t K,
                                   int32_t dim, const double* M, const double* w, int64_t scratch_bytes /* 0 = default */,
                                   int64_t enc_scratch_bytes /* 0 = default */, ssn_decoder** out);

/* Recall of a learned associative memory on the device (additive to ABI 11; csrc/ssn_recall.hip): for the dense
 * population whose scaled encoders are buffer `enc_buffer` (n x d_key, the matrix Voja moves) and one of whose outgoing
 * connections has the decoders `dec_buffer` (d_val x n, the matrix PES moves), and for n_keys key rows V (host doubles, C order),
 *   J[l][m] = scale[m] (V[l] . E[m]) + bias[m],   a = rate(J),   q[l][r] = sum_m W[r][m] a[l][m]
 * with rate(J) = amplitude / (tau_ref + tau_rc log1p(1 / (J - 1))) for J > 1, else 0 (SSN_LIF, SSN_LIFRATE) or
 * amplitude max(J, 0) (SSN_RELU).  scale = gain gives the reference scripts' recall (slam_map_new.py:342-347), scale = 1 the rates
 * the population really has for that key.  Both matrices are read where the simulator keeps them, in whichever layout the plan
 * chose, in their state at the time of the call; ssn_recall_run runs on the simulator's own stream, so it belongs between two
 * ssn_run_steps calls, and fills dst (n_keys x d_val host doubles) before it returns.  scale and bias (n host doubles; zero for
 * padded neurons, which then contribute nothing), the neuron constants and the keys are uploaded at creation; ssn_recall_set_keys
 * replaces the keys (any number of rows).  f32 simulators use the f32 matrix cores for both products; the decoder product is cut
 * into partial sums of 256 neurons that are added in ascending order, the scratch area (scratch_bytes, 0 = all partials up to
 * 64 MB, at least ssn_recall_info.min_scratch_bytes) only decides how many are kept at a time: the result does not depend on it
 * and is the same from run to run.  f64 simulators use plain ordered sums.  A recall must be destroyed before its simulator.
 * SSN_EINVAL: null handle or argument, n_keys == 0, a buffer that is not the shape claimed, scratch too small for one partial;
 * SSN_EUNSUPPORTED: a buffer of an ensemble array; SSN_EHIP "no HIP device available (there is no CPU fallback)" without a GPU. */
typedef struct ssn_recall ssn_recall;
typedef struct ssn_recall_info {
  int64_t n, d_key, d_val, n_keys;
  int64_t padded_keys;        /* key rows on the device (whole 64-row tiles)                                     */
  int64_t chunk;              /* neurons per partial sum of the decoder product (256)                            */
  int64_t n_chunks;
  int64_t chunks_per_pass;    /* partial sums the scratch area holds at a time                                   */
  int64_t scratch_bytes;
  int64_t min_scratch_bytes;  /* one partial sum                                                                 */
  int64_t dec_neuron_major;   /* 1: the decoders lie neuron-major [n][ldt] (spike-sparse plan), 0: row-major     */
  int64_t last_launches;      /* kernel launches of the last ssn_recall_run                                      */
  double last_kernel_ms;      /* their device time (HIP events around the kernels, the copy outside)             */
} ssn_recall_info;
int ssn_recall_create(ssn_sim* sim, int32_t enc_buffer, int32_t dec_buffer, int64_t n, int64_t d_key, int64_t d_val,
                      const double* scale, const double* bias, int32_t neuron, double tau_rc, double tau_ref, double amplitude,
                      const double* keys, int64_t n_keys, int64_t scratch_bytes /* 0 = default */, ssn_recall** out);
void ssn_recall_destroy(ssn_recall* rc);
int ssn_recall_set_keys(ssn_recall* rc, const double* keys, int64_t n_keys);
int ssn_recall_run(ssn_recall* rc, double* dst);
int ssn_recall_get_info(ssn_recall* rc, ssn_recall_info* out);

/* Binding of rows on the device (additive to ABI 11; csrc/ssn_bind.hip): out[r] = a[ra] (*) b[rb], the circular
 * convolution SSPSpace.bind / SPSpace.bind compute as ifft(fft(a) * fft(b)).real.  A binder depends on d and the dtype only, has a
 * stream and a scratch area of its own (0 = 64 MB; at least ssn_binder_info.min_scratch_bytes, one row) and is independent of
 * ssn_sim.  SSN_F32: one workgroup per row runs the whole convolution in LDS - both rows packed into one complex transform after
 * their norms are balanced by a power of two, the spectra separated and multiplied, one transform back (k_bind_rows); d with prime
 * factors <= 32 up to 6400 directly, any other d through the chirp-z form of a smooth length M >= 2 d - 1, M <= 6400.  SSN_F64 (the
 * parity mode): every entry the fma chain over i = 0 .. d - 1 of a_i b_{(j - i) mod d}, d <= 10000 (k_bind_direct).  Any other d is
 * SSN_EUNSUPPORTED.  flags: SSN_BIND_INVERT_A / _B read that operand at (d - i) mod d; SSN_BIND_NORMALIZE divides every output row
 * by max(its norm, norm_floor).  Pairing: an operand with a_n (b_n) rows gives output row r its row 0 (count 1), r (count n) or
 * r / (n / count) (count a divisor of n: one pose row for the L landmark rows of its sample); any other count is SSN_EINVAL.
 * ssn_binder_bind: dense host doubles in and out (the binder's dtype widened).  ssn_binder_bind_device: operands on the host or on
 * the binder's device, SSN_F32 / SSN_F64, leading dimensions >= d (elements) -> a device buffer of the binder's dtype with leading
 * dimension out_ld >= d, complete when the call returns; nothing outside the n x d entries is written.  n == 0 succeeds and writes
 * nothing.  The bits are the same for any scratch size, for host and device operands of the same values and from run to run.
 * Without a GPU: SSN_EHIP "no HIP device available (there is no CPU fallback)". */
enum ssn_bind_flag { SSN_BIND_INVERT_A = 1, SSN_BIND_INVERT_B = 2, SSN_BIND_NORMALIZE = 4 };
typedef struct ssn_binder ssn_binder;
typedef struct ssn_binder_info {
  int64_t row_chunk;          /* output rows per chunk                                                           */
  int64_t n_chunks;           /* chunks of a call with n rows                                                    */
  int64_t scratch_bytes;
  int64_t min_scratch_bytes;  /* one row: two staged operands and the host output, d doubles each                */
  int64_t d;
  int64_t transform_length;   /* L: points of the transforms run (M, or d); d for SSN_F64, which runs none       */
  int64_t bluestein_m;        /* M of the chirp-z form, 0 when d is transformed directly                         */
  int64_t n_radices;
  int64_t radices[12];        /* the Stockham passes of one transform of L points                                */
  int64_t threads;            /* per workgroup                                                                   */
  int64_t lds_bytes;          /* dynamic LDS per workgroup                                                       */
  int64_t last_launches;      /* kernel launches of the last bind call                                           */
  double last_kernel_ms;      /* their device time (HIP events around the kernels, copies outside)               */
} ssn_binder_info;
int ssn_binder_create(int32_t dtype, int32_t device, int64_t d, int64_t scratch_bytes /* 0 = default */, ssn_binder** out);
void ssn_binder_destroy(ssn_binder* binder);
int ssn_binder_bind(ssn_binder* binder, const double* a, int64_t a_n, const double* b, int64_t b_n, int64_t n, int32_t flags,
                    double norm_floor, double* out);
int ssn_binder_bind_device(ssn_binder* binder, const void* a, int32_t a_on_device, int32_t a_dtype, int64_t a_ld, int64_t a_n,
                           const void* b, int32_t b_on_device, int32_t b_dtype, int64_t b_ld, int64_t b_n, int64_t n, int32_t flags,
                           double norm_floor, void* out_dev, int64_t out_ld);
int ssn_binder_get_info(ssn_binder* binder, int64_t n, ssn_binder_info* out);

int ssn_get_counters(ssn_sim* sim, ssn_counters* out);
/* Fills at most `capacity` entries; returns the number of kernels with timed launches (or a negative status). */
int ssn_get_kernel_times(ssn_sim* sim, ssn_kernel_time* out, int32_t capacity);
int64_t ssn_n_steps(ssn_sim* sim);
int ssn_device_count(void);
const char* ssn_last_error(void);
const char* ssn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SSN_H */
