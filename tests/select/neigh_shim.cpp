// C entry points to the host-side decisions of the neighbourhood shrinkage (csrc/ndwt_select.h: neigh_tx, neigh_ty, neigh_geometry) for
// tests/test_neigh_select.py, tests/test_emulated_neigh.py and tests/test_gpu_neigh.py
// (host C++ only: g++ -std=c++17 -Wall -Wextra -Werror -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

// the tile of NeighShrink<T, COMP, nd, r>: elem_bytes = sizeof(T) * COMP
extern "C" int sel_neigh_tx(int nd) { return neigh_tx(nd); }
extern "C" int sel_neigh_ty(int nd, int elem_bytes, int r) { return neigh_ty(nd, elem_bytes, r); }
// workgroups per compute unit below which the march is split
extern "C" int sel_neigh_rounds() { return kNeighRounds; }
// out[4]: ntx, nty, chunk, nchunks
extern "C" void sel_neigh_geometry(int nd, long long n0, long long n1, long long n2, int elem_bytes, int r, long long blocks, int num_cus, int target_blocks,
                                   long long* out) {
    const NeighGeom g = neigh_geometry(nd, n0, n1, n2, elem_bytes, r, blocks, num_cus, target_blocks);
    out[0] = g.ntx;
    out[1] = g.nty;
    out[2] = g.chunk;
    out[3] = g.nchunks;
}
