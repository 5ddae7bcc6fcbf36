// Launch functions the kernel translation unit (tu_kernel.hip, one object per entry of PINKHIP_FAMILIES) exports to the
// host side of the library (pinkhip.hip), and the lookup from a launch plan to its function.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dispatch.h"
#include "ik_common.h"

namespace pinkhip {

struct RolloutArgs;
struct RolloutPairsArgs;

// The argument struct of the family that plans of KIND launch
#define PINKHIP_FAMILY(KIND, DENSE, PREFIX, ARGS, TABLE) ARGS launch_args_of(std::integral_constant<int, KIND>);
PINKHIP_FAMILIES(PINKHIP_FAMILY)
#undef PINKHIP_FAMILY
template <int KIND>
using LaunchArgs = decltype(launch_args_of(std::integral_constant<int, KIND>{}));

// Defined in tu_kernel.hip and explicitly instantiated there, once per object <prefix>_<NV>_<MD>_<W>.o: other units only
// name the instantiations (find_launcher below)
template <int KIND, int NV, int MD, int W, int DENSE>
hipError_t launch_entry(hipStream_t stream, const LaunchArgs<KIND> &a);

template <class Args>
using LaunchFn = hipError_t (*)(hipStream_t, const Args &);
template <class Want, class Have>
constexpr LaunchFn<Want> if_takes(LaunchFn<Have> f) {
  if constexpr (std::is_same_v<Want, Have>) return f;
  return nullptr;
}

// The launcher of plan `p` (NULL: none -- no such entry, or its family takes other arguments than Args)
template <class Args>
LaunchFn<Args> find_launcher(const LaunchPlan &p) {
#define PINKHIP_ROW(NV_, MD_, W_) \
  if (p.NV == NV_ && p.MD == MD_ && p.W == W_) return if_takes<Args, LaunchArgs<K>>(&launch_entry<K, NV_, MD_, W_, D>);
#define PINKHIP_FAMILY(KIND, DENSE, PREFIX, ARGS, TABLE) \
  if (p.kind == KIND && p.dense == DENSE) {              \
    constexpr int K = KIND, D = DENSE;                   \
    TABLE(PINKHIP_ROW)                                   \
  }
  PINKHIP_FAMILIES(PINKHIP_FAMILY)
#undef PINKHIP_FAMILY
#undef PINKHIP_ROW
  return nullptr;
}

}  // namespace pinkhip
