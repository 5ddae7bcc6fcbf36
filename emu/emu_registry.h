// Registry of the emulator's per-lane kernel entry points -- TEST INFRASTRUCTURE ONLY.  The slices of emu_part.cpp register
// the instantiations of their share of dispatch.h's tables at load time, under the PlanKind that launches them;
// emu_kernels.cpp looks them up where the library's launcher would pick a kernel.
#pragma once

namespace pinkemu {

typedef void (*LaneEntry)(void *);

void emu_register(int kind, int nv, int md, int w, LaneEntry fn);
LaneEntry emu_lookup(int kind, int nv, int md, int w);

}  // namespace pinkemu
