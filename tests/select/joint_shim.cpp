// C entry points to the host-side decisions of the joint shrinkage and the group norms (csrc/ndwt_select.h: joint_chunks and the
// constants the rule is written in) for tests/test_joint_select.py and tests/test_gpu_joint.py
// (host C++ only: g++ -std=c++17 -Wall -Wextra -Werror -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// workgroups per band of JointShrink / GroupNorms
extern "C" long long sel_joint_chunks(long long item_scalars, int comp, int vec, long long bands, long long items, int num_cus, int target_blocks) {
    return joint_chunks(item_scalars, comp, vec != 0, bands, items, num_cus, target_blocks);
}
// the steps every thread keeps before a band gets a further chunk are max(1, turns / items)
extern "C" int sel_joint_turns() { return kSelectTurns; }
// the items JointShrink keeps in registers
extern "C" int sel_joint_reg() { return kJointReg; }
