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

// Composite records (o_cmp): 16 doubles each.  A config lane reads its group's record as 16-byte words, and on the 64 banks of the
// LDS array the records of groups g and g' share banks when their starts are equal modulo 32 doubles: 16 doubles apart that is every
// second group (up to five distinct addresses on four banks for the puppet's nine groups).  kCmpStride = 18 doubles apart the starts
// are distinct modulo 32 for sixteen groups in a row and stay even, so the words stay 16-byte aligned.  The schedule (composite_form)
// takes the wide stride where the twist records behind the composites still fit the J area with it -- a system never loses the
// world-frame evaluation to it -- and 16 otherwise; the kernels read the stride back from the plan, (o_csw - o_cmp) / n_cgroups.
constexpr int kCmpRecord = 16, kCmpStride = 18;
static_assert(kCmpStride >= kCmpRecord && kCmpStride % 2 == 0 && kCmpRecord % 2 == 0, "composite records: 16-byte aligned");
template <class SP> constexpr int cmp_stride() {
    static_assert(SP::n_cgroups > 0 && (SP::o_csw - SP::o_cmp) % SP::n_cgroups == 0, "composite records: o_csw is not a whole number of strides behind o_cmp");
    constexpr int stride = (SP::o_csw - SP::o_cmp) / SP::n_cgroups;
    static_assert((stride == kCmpRecord || stride == kCmpStride) && (SP::o_cmp & 1) == 0, "composite records: stride");
    return stride;
}

}  // namespace tg

// A plain host compiler (the emulation of the kernels under tests/) also gets the compiler, whose HostProgram drives the emulated
// kernels; the kernel translation units, built by hipcc, get DevProg alone.
#ifndef __HIPCC__
#include "schedule.hpp"
#endif
