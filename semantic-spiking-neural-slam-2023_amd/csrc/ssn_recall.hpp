// ssn_recall.hpp - what ssn_recall.hip may see of a simulator (ssn_host.hip owns ssn_sim): where a matrix buffer lies on the
// device, in which layout, and the stream its kernels run on.  Nothing is copied; the view is valid while the simulator lives.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ssn_sim;

namespace ssn {

struct BufView {
  void* d = nullptr;         // device storage, elements of `dtype`
  int dtype = 0;             // SSN_F32 / SSN_F64: the simulator's
  int device = 0;
  hipStream_t stream = nullptr;      // the simulator's own stream
  int64_t rows = 0, cols = 0;        // logical shape
  int64_t ld = 0;                    // row-major [rows][ld] ...
  int transposed = 0;                // ... or neuron-major [cols][ldt] (Buf::transposed, the spike-sparse decoders)
  int64_t ldt = 0;
};

// SSN_OK and the view, or SSN_EINVAL (null simulator, id out of range, not a matrix of reals, a stream-ordered run in flight) /
// SSN_EUNSUPPORTED (a packed or re-ordered ensemble-array buffer); sets ssn_last_error.
int sim_buffer_view(ssn_sim* sim, int id, BufView* out);

}  // namespace ssn
