// ssn_encode.hpp - what csrc/ssn_decode.hip needs of the encoder of csrc/ssn_encode.hip beyond include/ssn.h.
#pragma once
#include <stdint.h>
#include "../../include/ssn.h"

namespace ssn {

// Encode n host points (n x dim doubles, dense) into a device buffer of `out_dtype` with leading dimension out_ld >= d, on the
// encoder's stream, chunk by chunk through its scratch area; returns when the buffer is complete.  An f64 encoder may write f32
// (every entry the float64 chain, rounded once): that is how a decoder's table is made.  An f32 encoder writes f32 only.
int encoder_encode_into(ssn_encoder* enc, const double* points, int64_t n, void* out_dev, int32_t out_dtype, int64_t out_ld);

}  // namespace ssn
