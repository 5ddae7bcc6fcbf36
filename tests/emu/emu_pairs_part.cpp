// One slice of the sphere-pair instantiations of the CPU wave emulator -- TEST INFRASTRUCTURE ONLY.
//   g++ -c -DEMU_PART=k -DEMU_NPARTS=n emu_pairs_part.cpp    for k = 0 .. n-1 (built in parallel, like emu_part.cpp)
#include "emu_pairs.h"

#ifndef EMU_PART
#define EMU_PART 0
#endif
#ifndef EMU_NPARTS
#define EMU_NPARTS 1
#endif

namespace {

// (the entries of the table are dealt out in turn)
template <int P, int I>
constexpr bool mine() {
  return (I % EMU_NPARTS) == P;
}

template <int P>
void register_slice() {
  using namespace pinkemu;
  constexpr int base = __COUNTER__ + 1;
#define PINKHIP_CASE(NV, MD, W) \
  if constexpr (mine<P, __COUNTER__ - base>()) emu_pairs_register(NV, MD, W, &lane_main_rollout_pairs<NV, MD, W>);
  PINKHIP_RPAIRS_TABLE(PINKHIP_CASE)
#undef PINKHIP_CASE
}

struct Registrar {
  Registrar() { register_slice<EMU_PART>(); }
} registrar;

}  // namespace
