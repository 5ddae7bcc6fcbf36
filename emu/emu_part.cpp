// One slice of the heavy kernel instantiations of the CPU wave emulator -- TEST INFRASTRUCTURE ONLY.
//   g++ -c -DEMU_PART=k -DEMU_NPARTS=n emu_part.cpp    for k = 0 .. n-1 (__graft_entry__.py builds them in parallel)
#include "emu_lanes.h"

#ifndef EMU_PART
#define EMU_PART 0
#endif
#ifndef EMU_NPARTS
#define EMU_NPARTS 1
#endif

namespace {

// The entries of every table of PINKHIP_FAMILIES are dealt out in turn
// (dependent on the template parameter P so that the branches of the other slices are discarded, not instantiated)
template <int P, int I>
constexpr bool mine() {
  return (I % EMU_NPARTS) == P;
}

template <int P>
void register_slice() {
  using namespace pinkemu;
  constexpr int base = __COUNTER__ + 1;
#define PINKHIP_ROW(NV, MD, W) \
  if constexpr (mine<P, __COUNTER__ - base>()) emu_register(K, NV, MD, W, &lane_main<K, NV, MD, W>);
#define PINKHIP_FAMILY(KIND, DENSE, PREFIX, ARGS, TABLE) \
  if constexpr (DENSE == 0) {                            \
    constexpr int K = pinkhip::KIND;                     \
    TABLE(PINKHIP_ROW)                                   \
  }
  PINKHIP_FAMILIES(PINKHIP_FAMILY)
#undef PINKHIP_FAMILY
#undef PINKHIP_ROW
}

struct Registrar {
  Registrar() { register_slice<EMU_PART>(); }
} registrar;

}  // namespace
