// C entry points to csrc/ndwt_slabs.h for tests/test_slab_walk.py (host C++ only: g++ -std=c++17 -shared -fPIC)
#include "../../non-decimated_wavelets_amd/csrc/ndwt_slabs.h"
using namespace ndwt;

// z0[i], n[i] of the ndev slabs of an axis of N planes
extern "C" void slabs_partition(long long N, int ndev, long long* z0, long long* n) {
    const std::vector<SlabPart> parts = slab_partition(N, ndev);
    for (int i = 0; i < ndev; ++i) { z0[i] = parts[(size_t)i].z0; n[i] = parts[(size_t)i].n; }
}

static std::vector<SlabPart> parts_of(int np, const long long* z0, const long long* n) {
    std::vector<SlabPart> parts;
    for (int i = 0; i < np; ++i) parts.push_back({z0[i], n[i]});
    return parts;
}

// the runs of for_each_run over the given slabs, (owner, local plane, done, run) each, at most max_runs of them written to out.
// Returns the number of runs; kNoOwner with the plane in *orphan; -2 if fn's own result (asked for at run `stop_at`) did not come back.
extern "C" int slabs_runs(int np, const long long* z0, const long long* n, long long N, long long g, long long count, int max_runs, long long* out,
                          long long* orphan, int stop_at) {
    int runs = 0;
    const int rc = for_each_run(parts_of(np, z0, n), N, g, count, [&](size_t o, long long lp, long long done, long long run) {
        if (runs == stop_at) return 77;
        if (runs < max_runs) { out[4 * runs] = (long long)o; out[4 * runs + 1] = lp; out[4 * runs + 2] = done; out[4 * runs + 3] = run; }
        ++runs;
        return 0;
    }, orphan);
    if (rc == 77) return runs == stop_at ? runs : -2;
    return rc == 0 ? runs : rc;
}

extern "C" int slabs_owner(int np, const long long* z0, const long long* n, long long gp) { return owner_of(parts_of(np, z0, n), gp); }

// nbr[i] at `halo` planes of reach, written to out (at most np entries); returns their number
extern "C" int slabs_neighbours(int np, const long long* z0, const long long* n, long long N, int i, long long halo, int* out) {
    const std::vector<int> nbr = slab_neighbours(parts_of(np, z0, n), N, (size_t)i, halo);
    for (size_t k = 0; k < nbr.size() && k < (size_t)np; ++k) out[k] = nbr[k];
    return (int)nbr.size();
}
