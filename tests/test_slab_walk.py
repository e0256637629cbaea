"""The plane walk of the single-process multi-device plan, checked without a device: csrc/ndwt_slabs.h is plain C++ on integers
(the slab partition, owner_of, the neighbour sets and for_each_run, the one loop behind every halo copy and every scatter of
csrc/ndwt_multi.hip), reached through a small host shim (tests/select/slabs_shim.cpp, compiled with g++) and compared with a
plane-by-plane brute force written here."""
import ctypes
import importlib
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LL = ctypes.c_longlong
KNOOWNER = -1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/slabs_shim.cpp")
    out = str(tmp_path_factory.mktemp("slabs") / "libslabs_shim.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", "slabs_shim.cpp"), "-o", out],
                   check=True)
    lib = ctypes.CDLL(out)
    lib.slabs_partition.restype = None
    lib.slabs_partition.argtypes = [LL, ctypes.c_int, ctypes.POINTER(LL), ctypes.POINTER(LL)]
    lib.slabs_runs.argtypes = [ctypes.c_int, ctypes.POINTER(LL), ctypes.POINTER(LL), LL, LL, LL, ctypes.c_int, ctypes.POINTER(LL), ctypes.POINTER(LL), ctypes.c_int]
    lib.slabs_owner.argtypes = [ctypes.c_int, ctypes.POINTER(LL), ctypes.POINTER(LL), LL]
    lib.slabs_neighbours.argtypes = [ctypes.c_int, ctypes.POINTER(LL), ctypes.POINTER(LL), LL, ctypes.c_int, LL, ctypes.POINTER(ctypes.c_int)]
    return lib


def _arr(v):
    return (LL * len(v))(*v)


def _partition(shim, N, ndev):
    z0, n = (LL * ndev)(), (LL * ndev)()
    shim.slabs_partition(N, ndev, z0, n)
    return list(z0), list(n)


def _runs(shim, z0, n, N, g, count, stop_at=-1):
    """[(owner, local plane, done, run)] of for_each_run, or its failure as (code, plane)"""
    cap = count + 1
    out, orphan = (LL * (4 * cap))(), LL(-1)
    r = shim.slabs_runs(len(z0), _arr(z0), _arr(n), N, g, count, cap, out, ctypes.byref(orphan), stop_at)
    if r < 0:
        return r, orphan.value
    assert r <= cap
    return [tuple(out[4 * k:4 * k + 4]) for k in range(r)]


def _brute(z0, n, N, g, count):
    """(owner, local plane) of every plane, one at a time"""
    planes = []
    for k in range(count):
        gp = (g + k) % N                                         # Python's % is already the non-negative one
        own = [i for i in range(len(z0)) if z0[i] <= gp < z0[i] + n[i]]
        assert len(own) == 1, (N, z0, n, gp)
        planes.append((own[0], gp - z0[own[0]]))
    return planes


def _check_walk(shim, z0, n, N, g, count):
    runs = _runs(shim, z0, n, N, g, count)
    assert isinstance(runs, list), (N, z0, g, count, runs)
    flat, done = [], 0
    for k, (o, lp, d, run) in enumerate(runs):
        assert d == done and run >= 1, (N, z0, g, count, runs)
        assert 0 <= lp and lp + run <= n[o], (N, z0, g, count, runs)                  # inside one slab
        assert k == len(runs) - 1 or lp + run == n[o], (N, z0, g, count, runs)        # maximal: only the last run may stop short of its slab's end
        flat += [(o, lp + j) for j in range(run)]
        done += run
    assert done == count and flat == _brute(z0, n, N, g, count), (N, z0, g, count, runs)
    return len(runs)


def test_partition_agrees_with_the_python_driver(shim):
    sh = importlib.import_module("non-decimated_wavelets_amd.sharded")
    for N in range(1, 41):
        for ndev in range(1, min(N, 8) + 1):
            z0, n = _partition(shim, N, ndev)
            assert [(a, a + b) for a, b in zip(z0, n)] == sh.partition(N, ndev)
            assert all(b >= 1 for b in n) and z0[0] == 0 and z0[-1] + n[-1] == N
            for gp in range(-2, N + 2):
                want = [i for i in range(ndev) if z0[i] <= gp < z0[i] + n[i]]
                assert shim.slabs_owner(ndev, _arr(z0), _arr(n), gp) == (want[0] if want else -1)


def test_walk_matches_a_plane_by_plane_brute_force(shim):
    """every halo a level can ask for: both sides of every slab, 0 .. 2 N planes (several slabs away, longer than the axis)"""
    cases = runs = 0
    for N in range(1, 41):
        for ndev in range(1, min(N, 8) + 1):
            z0, n = _partition(shim, N, ndev)
            for halo in range(0, 2 * N + 1):
                for i in range(ndev):
                    runs += _check_walk(shim, z0, n, N, z0[i] - halo, halo)           # before the slab
                    runs += _check_walk(shim, z0, n, N, z0[i] + n[i], halo)           # after it
                    cases += 2
    assert cases == sum(2 * ndev * (2 * N + 1) for N in range(1, 41) for ndev in range(1, min(N, 8) + 1))
    assert runs > cases                                          # (multi-run walks were among them)


def test_walk_of_a_slab_with_its_halos_and_of_gather_lengths(shim):
    """the in-line analysis copy and the gather synthesis walk halo + n + halo planes in one call"""
    for N in range(1, 25):
        for ndev in range(1, min(N, 8) + 1):
            z0, n = _partition(shim, N, ndev)
            for before in range(0, N + 2):
                for i in range(ndev):
                    _check_walk(shim, z0, n, N, z0[i] - before, before + n[i] + before + 1)


def test_neighbour_sets(shim):
    for N in range(1, 41):
        for ndev in range(1, min(N, 8) + 1):
            z0, n = _partition(shim, N, ndev)
            for halo in range(0, 2 * N + 1):
                for i in range(ndev):
                    out = (ctypes.c_int * ndev)()
                    k = shim.slabs_neighbours(ndev, _arr(z0), _arr(n), N, i, halo, out)
                    assert 1 <= k <= ndev
                    got = list(out[:k])
                    want = []                                    # owners of the planes within halo of the slab, in the order they are met
                    for o, _ in _brute(z0, n, N, z0[i] - halo, n[i] + 2 * halo):
                        if o not in want:
                            want.append(o)
                    assert got == want and i in got, (N, ndev, halo, i, got, want)


def test_walk_reports_a_plane_without_owner_and_passes_an_error_through(shim):
    # planes 4 and 5 of an axis of 8 belong to nobody
    z0, n = [0, 6], [4, 2]
    assert _runs(shim, z0, n, 8, 2, 5) == (KNOOWNER, 4)
    assert _runs(shim, z0, n, 8, -2, 5) == [(1, 0, 0, 2), (0, 0, 2, 3)]
    # fn's own non-zero result ends the walk at that run and comes back unchanged (the shim answers with the number of runs before it)
    z0, n = _partition(shim, 12, 3)
    assert len(_runs(shim, z0, n, 12, -5, 29)) == 8
    for stop in range(8):
        out, orphan = (LL * 64)(), LL(-1)
        assert shim.slabs_runs(3, _arr(z0), _arr(n), 12, -5, 29, 16, out, ctypes.byref(orphan), stop) == stop
