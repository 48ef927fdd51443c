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

// Carried poses (schedule.hpp, pose_carry): whether the rollout kernel of a system may take the midpoint and q2 poses of
// a step's first evaluation behind the step edge from the q2 poses the converged evaluation before it left in LDS, and what it needs for
// it.  NOT a member of DevProg: the generic kernels never read it, and a specialisation header gains its cells (pc_on, pc_n, pc_kin_0 /
// pc_kin_1, pc_item) only where it is on -- the header of every other system stays the text it was, and with it its kernels.
//   item[i]: the (set 1, joint) item, in sj_list's layout, of a joint whose midpoint pose is read but whose q2 pose is not (no q2 twin in
//            sj_list): the local-transform pass gives it to lane n_sj + i, so that the chain step which already runs over it in pose set 1
//            leaves its q2 world pose in G2
//   kin:     bit l set when item l of sj_list is a joint that a kinematic config moves (a translation-run joint, by the conditions)
constexpr int kPoseCarryMax = 8;
struct PoseCarry {
    int on = 0, n = 0;
    int item[kPoseCarryMax] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned kin[2] = {0u, 0u};
};

}  // namespace tg

// A plain host compiler (the emulation of the kernels under tests/) also gets the compiler, whose HostProgram drives the emulated
// kernels; the kernel translation units, built by hipcc, get DevProg alone.
#ifndef __HIPCC__
#include "schedule.hpp"
#endif
