// The point transform every kernel that must return the reference's bits shares: the NDT derivative pass (ndt_point.hpp, and with
// it the host emulation tools/ndt_host_emu) and the sensor-frame transform of the raw scan (cloud_codec.hip).  A header of its own
// so that a unit compiled under another contraction rule can include it: the function forbids contraction itself.
#pragma once

namespace lsr {

// Point transform in the REFERENCE's rounding order — pcl::transformPointCloud: ((m00 x + m01 y) + m02 z) + m03, every product
// and sum rounded to fp32, no fused multiply-add.  The order matters more than it looks: a coordinate of ~50 m carries an
// fp32 rounding error of ~2e-6 m, q = x' - mean is ~1 m, and the gradient of a pass moves by 3e-7 (relative) between this
// order and an fmaf chain — enough to send a registration that walks thirty clamped 0.1 m steps along an ill-conditioned
// Newton direction (BASELINE cfg 4, candidate 21) 2.4 mm away from the reference's result (tests/test_ndt_host_emu_cpu.py).
__device__ __forceinline__ float xform_ref(const float a, const float b, const float c, const float d, const float x, const float y,
                                           const float z) {
#pragma clang fp contract(off)
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z)), d);
}

}  // namespace lsr
