// C entry points to the host-side decisions of the tile form of the joint shrinkage and the group norms (csrc/ndwt_select.h: joint_route,
// joint_tile_strips and the constants the rule is written in) for tests/test_joint_tile_select.py and tests/test_gpu_joint_tile.py
// (host C++ only: g++ -std=c++17 -Wall -Wextra -Werror -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// 1: the tile form (JointTile / GroupNormsTile), 0: the chunk form (JointShrink / GroupNorms)
extern "C" int sel_joint_route(long long item_scalars, int comp, int vec, long long bands, long long items, int num_cus, int variant_inv) {
    return joint_route(item_scalars, comp, vec != 0, bands, items, num_cus, variant_inv) == kJointTile;
}
// workgroups per band of the tile form
extern "C" long long sel_joint_tile_strips(long long item_scalars, int comp, int vec) { return joint_tile_strips(item_scalars, comp, vec != 0); }
// the steps of a strip and the items of an LDS tile
extern "C" int sel_joint_tile_sw() { return kJointTileSW; }
extern "C" int sel_joint_tile_j() { return kJointTileJ; }
// below this many items the tile form is never taken unasked
extern "C" long long sel_joint_tile_from() { return kJointTileFrom; }
