// program.hpp -- the flat device schedule of one system: what the host's topology compiler (schedule.hpp) hands to the kernels.
#pragma once
#include "../../include/trep_amd.h"

namespace tg {

// Plain-old-data view handed to the kernels (device pointers when on the GPU).  Its members are listed, and documented, in
// devprog_fields.def: the sizes, counts and LDS offsets first, then one pointer per table.
struct DevProg {
#define TG_F_INT(name) int name;
#define TG_F_ARRAY(type, name, n) type name[n];
#define TG_F_TABLE(type, name) const type *name;
#include "devprog_fields.def"
#undef TG_F_INT
#undef TG_F_ARRAY
#undef TG_F_TABLE
};

}  // namespace tg

// A plain host compiler (the emulation of the kernels under tests/) also gets the compiler, whose HostProgram drives the emulated
// kernels; the kernel translation units, built by hipcc, get DevProg alone.
#ifndef __HIPCC__
#include "schedule.hpp"
#endif
