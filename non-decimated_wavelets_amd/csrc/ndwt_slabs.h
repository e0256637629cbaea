// ndwt_slabs.h -- the slabs of a sharded axis and the walk over its planes: plain host C++ on integers (no HIP header; any host
// compiler takes it).  ndwt_multi.hip cuts the axis here and moves every run of planes through for_each_run;
// tests/test_slab_walk.py checks the walk plane by plane through tests/select/slabs_shim.cpp, without a device.
#pragma once
#include <stddef.h>

#include <vector>

namespace ndwt {

struct SlabPart { long long z0, n; };   // planes [z0, z0 + n) of the sharded axis

// N planes over ndev slabs, uneven remainders allowed (sharded.partition of the Python driver)
inline std::vector<SlabPart> slab_partition(long long N, int ndev) {
    std::vector<SlabPart> parts;
    for (int i = 0; i < ndev; ++i) {
        const long long z0 = (long long)i * N / ndev;
        parts.push_back({z0, (long long)(i + 1) * N / ndev - z0});
    }
    return parts;
}

// `parts`: any indexable container of objects with z0 and n (SlabPart, or the Slab of ndwt_multi.hip).  The index of the slab that
// holds plane gp, -1 if none does.
template <class Parts> inline int owner_of(const Parts& parts, long long gp) {
    for (size_t i = 0; i < parts.size(); ++i)
        if (gp >= parts[i].z0 && gp < parts[i].z0 + parts[i].n) return (int)i;
    return -1;
}

constexpr int kNoOwner = -1;   // for_each_run: a plane that no slab holds (the parts do not cover the axis); never a result of fn

// The `count` planes that start at global plane g of a periodic axis of N planes (g may be negative or beyond N, count longer than N),
// cut into maximal runs inside one slab: fn(owner index, local plane in the owner, planes done so far, run length) for every run, in
// order.  Stops at the first fn that does not return 0 and returns its result; kNoOwner with the plane in *orphan for a plane without owner.
template <class Parts, class Fn> inline int for_each_run(const Parts& parts, long long N, long long g, long long count, Fn&& fn, long long* orphan = nullptr) {
    for (long long done = 0; done < count;) {
        const long long gp = ((g + done) % N + N) % N;
        const int o = owner_of(parts, gp);
        if (o < 0) {
            if (orphan) *orphan = gp;
            return kNoOwner;
        }
        long long run = parts[(size_t)o].z0 + parts[(size_t)o].n - gp;
        if (run > count - done) run = count - done;
        const int rc = fn((size_t)o, gp - parts[(size_t)o].z0, done, run);
        if (rc != 0) return rc;
        done += run;
    }
    return 0;
}

// nbr[i]: the slabs (i itself included) that own a plane within `halo` planes of slab i, in the order the walk from z0 - halo meets them
template <class Parts> inline std::vector<int> slab_neighbours(const Parts& parts, long long N, size_t i, long long halo) {
    std::vector<int> nbr;
    for_each_run(parts, N, parts[i].z0 - halo, parts[i].n + 2 * halo, [&](size_t o, long long, long long, long long) {
        bool have = false;
        for (int q : nbr) have = have || q == (int)o;
        if (!have) nbr.push_back((int)o);
        return 0;
    });
    return nbr;
}

}  // namespace ndwt
