// brs_nan.hpp -- the NaN rule of the float actors, critics and learners in one place: the selects of their tails
// written so that a NaN operand comes back as a NaN, as np.clip, np.maximum, torch.relu, torch.clamp and torch.min return it.
// fminf / fmaxf (v_min_f32 / v_max_f32) return the OTHER operand, and a compare with a NaN is false, so `x > 0 ? x : 0` is 0: a
// diverged network would leave such a tail as a finite number that nothing downstream can tell from a healthy one.  Every
// function returns, for operands that are not NaN, the bytes of the expression it replaces.  The translation units that include
// this are built without -ffast-math (_lib.py: UNITS), so the compares are honest.  Compiles with g++.
#pragma once
#include <math.h>

#ifndef BRS_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BRS_HD __host__ __device__ __forceinline__
#else
#define BRS_HD inline
#endif
#endif

namespace brs {

// np.clip / torch.clamp: fminf(hi, fmaxf(lo, a)) where a is a number
BRS_HD float clip_keep_nan(float a, float lo, float hi) { return a != a ? a : fminf(hi, fmaxf(lo, a)); }
// np.minimum / torch.min: fminf(a, b) where both are numbers
BRS_HD float min_keep_nan(float a, float b) { return a != a ? a : (b != b ? b : fminf(a, b)); }
// np.maximum(x, 0) / torch.relu: +0 for x <= 0 (either zero), x above, NaN for NaN
BRS_HD float relu_keep_nan(float x) { return x <= 0.0f ? 0.0f : x; }
// torch's threshold_backward lets the gradient through unless the pre-activation (equivalently: the ReLU's output) is <= 0: a
// NaN keeps the gate open, so that the NaN of its row reaches the sums
BRS_HD bool relu_gate_keep_nan(float pre) { return !(pre <= 0.0f); }

}  // namespace brs
