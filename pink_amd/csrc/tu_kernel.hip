// The one launcher translation unit: compiled once per entry of every table of PINKHIP_FAMILIES (dispatch.h) with
//   -DPINKHIP_TU_FAMILY=<prefix> -DPINKHIP_TU_NV=<NV> -DPINKHIP_TU_MD=<MD> -DPINKHIP_TU_W=<W>       (Makefile)
// The fully unrolled register-resident rows make every instantiation a long compile; as separate objects they build in
// parallel and only the host file is touched by an ABI change.  What differs between the families is their
// pinkhip::Family, next to each kernel; templates that are not instantiated add nothing to the code object.
#include <hip/hip_runtime.h>

#include <cstdlib>

// clang-format off
#define PINKHIP_NO_ELEMENTWISE_KERNELS
#include "wave.h"
#include "ik_rollout.h"
#include "launchers.h"
// clang-format on

#if !defined(PINKHIP_TU_FAMILY) || !defined(PINKHIP_TU_NV) || !defined(PINKHIP_TU_MD) || !defined(PINKHIP_TU_W)
#error "tu_kernel.hip is compiled once per (family, NV, MD, W): see the Makefile"
#endif

namespace pinkhip {

#define PINKHIP_CAT_(a, b) a##b
#define PINKHIP_CAT(a, b) PINKHIP_CAT_(a, b)
#define PINKHIP_FAMILY(KIND, DENSE, PREFIX, ARGS, TABLE) constexpr int kKind_##PREFIX = KIND, kDense_##PREFIX = DENSE;
PINKHIP_FAMILIES(PINKHIP_FAMILY)
#undef PINKHIP_FAMILY
constexpr int kKind = PINKHIP_CAT(kKind_, PINKHIP_TU_FAMILY), kDense = PINKHIP_CAT(kDense_, PINKHIP_TU_FAMILY);

template <int KIND, int NV, int MD, int W, int DENSE>
hipError_t launch_entry(hipStream_t stream, const LaunchArgs<KIND> &a) {
  using F = Family<KIND, NV, MD, W, DENSE != 0>;
  constexpr int G = kWave / W;
  const typename F::Args k = F::prepared(a);
  size_t lds = F::lds_bytes(k);
#ifdef PINKHIP_SECTION_CLOCK
  // profiling builds only: PINKHIP_LDS_TOTAL=<bytes> asks for more LDS per wave to lower the occupancy (40000: one
  // wave per SIMD, 20000: two) -- per-section cycles of a wave that runs alone vs. among three
  if (KIND == PLAN_PACKED)
    if (const char *t = std::getenv("PINKHIP_LDS_TOTAL")) lds = static_cast<size_t>(std::atoll(t)) > lds ? static_cast<size_t>(std::atoll(t)) : lds;
#endif
  const dim3 grid(static_cast<unsigned>((F::B(k) + G - 1) / G)), block(kWave);
  hipLaunchKernelGGL(F::kernel, grid, block, lds, stream, k);
  return hipGetLastError();
}
template hipError_t launch_entry<kKind, PINKHIP_TU_NV, PINKHIP_TU_MD, PINKHIP_TU_W, kDense>(hipStream_t, const LaunchArgs<kKind> &);

}  // namespace pinkhip

#if defined(PINKHIP_SECTION_CLOCK) && PINKHIP_CAT(PINKHIP_CLOCK_, PINKHIP_TU_FAMILY)
// profiling builds only (scripts/section_clock.py: make DEV=1 SECTION_CLOCK=1 EXTRA=-DPINKHIP_CLOCK_<prefix>): the unit of
// that family exports the accessor that reads and clears the per-section cycle counters of its kernel
extern "C" int pinkhip_debug_section_clock(void *handle_unused, unsigned long long *out16) {
  (void)handle_unused;
  if (!out16) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(pinkhip_clock), 16 * sizeof(unsigned long long)) != hipSuccess) return -2;
  unsigned long long zero[16] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(pinkhip_clock), zero, sizeof(zero)) != hipSuccess) return -2;
  return 0;
}
#endif
