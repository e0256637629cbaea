// ndwt_multi.hip -- single-process, multi-device plan: ONE host thread drives the GPUs of a node.
//
// The reference's host is one MATLAB process calling one gateway (Functions/nd_dwt_3D.m:161,225 -> mex/nd_dwt_mex.c:8): a
// drop-in multi-GPU path has to live behind that single call.  This file shards the volume in slabs on its outermost axis
// over `devices[]` (a device may be listed several times: independent slabs and streams on one GPU -- how the path is tested on
// a one-GPU machine), runs the level loop with the slab entry points of include/ndwt.h and moves planes between slabs with
// asynchronous device-to-device copies (peer copies over xGMI when the slabs live on different GPUs).  Streams are ordered
// with events only; the host thread blocks once, at the end of a call.
//
// Data stays where it is: ndwt_mdec / ndwt_mrec take one device pointer per slab (the slab of x on its device, the band-planar
// coefficient slab on its device) and the kernels read and write them in place -- no plan-owned copy of a slab exists.  The host
// forms stage whole-volume host arrays through plan-owned slab buffers and call the same code.
//
// Overlap (round 4; ndwt_mplan_set_overlap, on by default): every slab has a second stream for its copies.  Analysis: the halo planes travel
// on the copy stream while the planes that need none of them are computed (one launch), then the two ends (one launch).  Scatter synthesis:
// the partial sums a slab owes its neighbours are computed FIRST (one launch for both margins), travel on the destinations' copy streams
// while every slab synthesises its own planes, and are added behind that launch.  Slabs are still joined by one event barrier per level.
//
// Exchange per level:
//   analysis   the halo planes of the approximation band only ((L/2-1) s before, (L/2) s after the slab), copied from their
//              owners into small buffers / the margins of the approximation scratch: bit-identical to one device.
//   synthesis  NDWT_EXCHANGE_SCATTER (default where the plan's levels run the fused kernels): every slab synthesises its own
//              coefficients zero-extended -- its n planes in place, plus the partial sums it owes the (L-1) s planes around it --
//              and those ONE-band planes are copied to their owners and added (a plane gets its addends in a fixed order, so
//              results are deterministic; they equal the single-device ones to rounding, the order of summation differs).
//              NDWT_EXCHANGE_GATHER: the halo planes of all 2^d bands are assembled with the slab in a scratch array (a copy of
//              every band per level) -- bit-identical to one device, and the path of plans whose levels run per-axis kernels.
//
// How the file is built:
//   one walk    "the planes from periodic global plane g, cut at the slabs' ends" is ndwt::for_each_run of ndwt_slabs.h (HIP-free, with the
//               slab partition and the neighbour sets; tested on the CPU).  walk() applies it to the plan's slabs and is the only place that
//               reports a plane without owner; every halo copy (copy_planes) and every scatter (scatter_margin, the destination side of
//               the overlapped synthesis) is a call of it.
//   one mover   move_planes copies or adds planes of every frame between two slabs: outermost-axis slabs (one frame) by asynchronous or
//               peer copies and add_planes_kernel, z-slabs of a 4-D volume (nt frames) by strided segment launches or a peer copy per frame.
//   one level loop per direction, for both kinds of slab (frame factor R, margin H): mdec_core and mrec_core work out a level's pointers
//               once and pick its step -- DecStep: overlapped, split-halo, in-line halo; RecStep: overlapped scatter, scatter by three
//               parts, scatter by zero-extended scratch (z-slabs), gather.  The plain scatter steps run on the caller's thread in slab
//               order, the overlapped steps and the analysis through phase(): the order of the event records depends on it.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../include/ndwt.h"
#include "ndwt_slabs.h"
#include "ndwt_trace.h"

namespace {

struct Slab {
    int device;
    long long z0, n;               // planes [z0, z0 + n) of the outer axis
    ndwt_plan* plan;
    hipStream_t stream;
    hipStream_t cstream;           // this slab's copies (halo planes in, partial sums in) when the exchange overlaps with compute
    hipEvent_t copied;             // "the copies queued on cstream for this level have arrived"
    hipEvent_t ready[2];           // "approximation buffer k of this slab is complete" (k = level parity)
    hipEvent_t margins;            // "the partial sums this slab owes its neighbours are computed" (scatter synthesis)
    char* approx[2];               // [halo_max | n | halo_max] planes each: the approximation band between levels
    char* hb;                      // level-1 analysis halos of a device-resident x: halo_max planes before ...
    char* ha;                      // ... and after the slab
    char* mb;                      // scatter synthesis: partial sums for the planes before the slab (halo_max planes) ...
    char* ma;                      // ... and after it
    char* recv;                    // scatter synthesis: planes received from the neighbours before they are added (2 * halo_max planes)
    long long recv_used;           // planes of recv handed out in the current level (overlapped schedule)
    char* gather;                  // gather synthesis: 2^d bands * (n + L - 1) planes, allocated on first use
    char* xbuf;                    // host forms: the slab of x / of the result, allocated on first use
    char* coef;                    // host forms: all bands of the slab, allocated on first use
};

template <typename T>
__global__ __launch_bounds__(256) void add_planes_kernel(T* __restrict__ dst, const T* __restrict__ src, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += step) dst[i] += src[i];
}

}  // namespace

// The host side of a call with several slabs: one thread per slab queues that slab's work (ONE thread queueing for 8 devices takes longer
// than a device needs to compute its share: 1.7 ms against 1.0 ms for cfg3 -- tools/mplan_host_time.py).  Slab 0 is the caller; the others
// are persistent workers that sleep between calls and spin between the phases of one (a phase = the same function for every slab, all
// slabs done before the next phase starts: what one slab's stream waits for must have been RECORDED by the host before the wait is queued).
struct Team {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv;
    bool stop = false;
    int call_gen = 0;                     // (under m) a call has begun: workers wake up and spin on phase_gen
    std::atomic<int> active{0};           // a call is in progress
    std::atomic<int> phase_gen{0};
    std::atomic<int> remaining{0};
    std::function<int(size_t)> job;
    std::vector<int> rc;
    std::vector<std::string> err;
    pid_t pid = 0;                        // the process that started the workers (a forked child has the plan but not the threads)
};

struct ndwt_mplan {
    int ndim, dtype, complexity, max_level, nb;
    long long dims[NDWT_MAX_DIMS];
    int shard;                     // the sharded axis: ndim - 1 (outermost), or 2 of a 4-D volume (z; t whole on every slab)
    long long nrep;                // frames: runs of planes per plane index of the sharded axis (1 for the outermost axis)
    size_t plane_bytes;            // bytes of one plane of the sharded axis (one band; z-slabs: of one frame)
    long long halo_max;            // planes of margin in the approximation buffers
    int L_outer;
    int dilation;
    int exchange;                  // NDWT_EXCHANGE_*
    int fast;                      // the slab plans offer the split-halo analysis and the zero-extended synthesis at tap stride 1
    int overlap;                   // copies on the slabs' copy streams, overlapped with the launches that do not wait for them
    std::vector<Slab> slabs;
    std::string notes;             // peer-access findings of plan creation (ndwt_mplan_describe)
    double last_enqueue_us;        // host time the last ndwt_mdec / ndwt_mrec spent queueing work (before it waited for the devices)
    int threads;                   // 1: one host thread per slab queues its work (default with more than one slab); 0: the caller queues everything
    Team* team;
    std::vector<std::pair<int, int>> peer;   // (a, b): kernels on device a may read device b's memory (peer access enabled)
    std::vector<std::vector<int>> nbr;   // nbr[i]: the slabs (i itself included) that own a plane within halo_max of slab i: the only slabs whose
                                         // buffers slab i ever reads or whose copies ever read slab i's (the relation is symmetric)
};

static thread_local std::string g_merr;

static int mfail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_merr = buf;
    return code;
}
#define MHIP(expr)                                                                                         \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return mfail(NDWT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)
#define MTRY(expr)                                                     \
    do {                                                               \
        int rc_ = (expr);                                              \
        if (rc_ != NDWT_OK) return mfail(rc_, "%s", ndwt_last_error()); \
    } while (0)
#define MRET(expr)                          \
    do {                                    \
        int rc_ = (expr);                   \
        if (rc_ != NDWT_OK) return rc_;     \
    } while (0)

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}

static void team_worker(ndwt_mplan* mp, size_t i) {
    Team& t = *mp->team;
    int seen_call = 0, seen_phase = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(t.m);
            t.cv.wait(lk, [&] { return t.stop || t.call_gen != seen_call; });
            if (t.stop) return;
            seen_call = t.call_gen;
        }
        while (t.active.load(std::memory_order_acquire)) {
            const int g = t.phase_gen.load(std::memory_order_acquire);
            if (g == seen_phase) { cpu_relax(); continue; }
            seen_phase = g;
            const int rc = t.job(i);
            t.rc[i] = rc;
            if (rc) t.err[i] = g_merr;
            t.remaining.fetch_sub(1, std::memory_order_release);
        }
    }
}

// a call begins: the workers wake up (created on the first call) and spin until team_end
static void team_begin(ndwt_mplan* mp) {
    const size_t G = mp->slabs.size();
    if (!mp->threads || G < 2) return;
    if (mp->team && mp->team->pid != getpid()) mp->team = nullptr;   // forked: the parent's workers do not exist here (its Team object is left alone)
    if (!mp->team) {
        mp->team = new Team();
        mp->team->pid = getpid();
        mp->team->rc.assign(G, 0);
        mp->team->err.assign(G, std::string());
        for (size_t i = 1; i < G; ++i) mp->team->th.emplace_back(team_worker, mp, i);
    }
    Team& t = *mp->team;
    t.active.store(1, std::memory_order_release);
    {
        std::lock_guard<std::mutex> lk(t.m);
        ++t.call_gen;
    }
    t.cv.notify_all();
}
static void team_end(ndwt_mplan* mp) {
    if (mp->team) mp->team->active.store(0, std::memory_order_release);
}
static void team_destroy(ndwt_mplan* mp) {
    if (!mp->team) return;
    if (mp->team->pid != getpid()) { mp->team = nullptr; return; }
    {
        std::lock_guard<std::mutex> lk(mp->team->m);
        mp->team->stop = true;
    }
    mp->team->cv.notify_all();
    for (auto& th : mp->team->th) th.join();
    delete mp->team;
    mp->team = nullptr;
}

// One phase of a call: fn(i) for every slab i -- concurrently, one host thread per slab, when the team is active; in slab order on the
// caller's thread otherwise.  Returns when every slab's fn has returned, with the first error (its message in this thread's g_merr).
// fn(i) touches slab i's streams only, and starts with hipSetDevice (the current device is per thread).
template <class F> static int phase(ndwt_mplan* mp, F&& fn) {
    const size_t G = mp->slabs.size();
    Team* t = mp->team;
    if (!t || !t->active.load(std::memory_order_relaxed)) {
        for (size_t i = 0; i < G; ++i) MRET(fn(i));
        return NDWT_OK;
    }
    t->job = [&fn](size_t i) -> int { return fn(i); };
    t->remaining.store((int)G - 1, std::memory_order_relaxed);
    t->phase_gen.fetch_add(1, std::memory_order_release);
    const int rc0 = fn(0);
    while (t->remaining.load(std::memory_order_acquire) != 0) cpu_relax();
    if (rc0) return rc0;
    for (size_t i = 1; i < G; ++i)
        if (t->rc[i]) { g_merr = t->err[i]; return t->rc[i]; }
    return NDWT_OK;
}

static long long stride_of(const ndwt_mplan* mp, int lev) { return mp->dilation == NDWT_DILATION_ATROUS ? (1LL << (lev - 1)) : 1LL; }

static long long axis_len(const ndwt_mplan* mp) { return mp->dims[mp->shard]; }

static bool z_slabs(const ndwt_mplan* mp) { return mp->shard != mp->ndim - 1; }

static size_t index_of(const ndwt_mplan* mp, const Slab& s) { return (size_t)(&s - &mp->slabs[0]); }

// band b >= 1 of level lev in a band-planar coefficient array of `level` levels (band 0: the approximation of the last level)
static long long band_index(const ndwt_mplan* mp, int level, int lev, int b) { return 1 + (long long)(mp->nb - 1) * (level - lev) + (b - 1); }

// The one walk over planes (ndwt::for_each_run of ndwt_slabs.h on the plan's slabs): the `count` planes from GLOBAL plane g (periodic) in
// maximal runs inside one slab, fn(owner index, local plane in the owner, planes done so far, run length) -> NDWT_OK or an error.
template <class Fn> static int walk(ndwt_mplan* mp, long long g, long long count, Fn&& fn) {
    long long orphan = 0;
    const int rc = ndwt::for_each_run(mp->slabs, axis_len(mp), g, count, fn, &orphan);
    return rc == ndwt::kNoOwner ? mfail(NDWT_ERR_INVALID_ARG, "plane %lld has no owner", orphan) : rc;
}

// kernels on to_dev may read from_dev's memory
static bool direct_access(const ndwt_mplan* mp, int to_dev, int from_dev) {
    if (to_dev == from_dev) return true;
    for (auto& pr : mp->peer)
        if (pr.first == to_dev && pr.second == from_dev) return true;
    return false;
}

// The one plane mover.  `planes` planes of every frame: dst (dst_fp planes per frame) = (op NDWT_SEG_COPY) or += (NDWT_SEG_ADD) src (src_fp
// planes per frame), on `to`'s stream st.  Slabs of the outermost axis are one frame (dst_fp, src_fp unused): an asynchronous copy, a peer
// copy between devices, or add_planes_kernel on a src in `to`'s memory.  z-slabs, nrep frames: one strided segment launch on the
// destination's device (ndwt_slab_segments_strided: it reads the source in place where the devices are the same or have peer access),
// else one peer copy per frame, and no add.
static int move_planes(ndwt_mplan* mp, Slab& to, char* dst, long long dst_fp, const Slab& from, const char* src, long long src_fp,
                       long long planes, int op, hipStream_t st) {
    const size_t pb = mp->plane_bytes, es = mp->dtype == NDWT_F32 ? 4 : 8;
    if (planes <= 0) return NDWT_OK;
    if (mp->nrep == 1 && op == NDWT_SEG_COPY) {
        const size_t bytes = (size_t)planes * pb;
        if (from.device == to.device) MHIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
        else MHIP(hipMemcpyPeerAsync(dst, to.device, src, from.device, bytes, st));
        return NDWT_OK;
    }
    if (mp->nrep == 1) {
        const long long n = (long long)((size_t)planes * pb / es);
        long long blocks = (n + 255) / 256;
        if (blocks > 256 * 32) blocks = 256 * 32;
        ndwt::trace_plain(dim3((unsigned)blocks), dim3(256), "add_planes_kernel", mp->dtype == NDWT_F32 ? "float" : "double");
        if (mp->dtype == NDWT_F32) hipLaunchKernelGGL(add_planes_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (float*)dst, (const float*)src, n);
        else hipLaunchKernelGGL(add_planes_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st, (double*)dst, (const double*)src, n);
        MHIP(hipGetLastError());
        return NDWT_OK;
    }
    if (direct_access(mp, to.device, from.device)) {
        const long long spp = (long long)(pb / es);       // scalars per plane
        void* d[1] = {dst};
        const void* sr[1] = {src};
        const int64_t cnt = planes * spp, ds = dst_fp * spp, ss = src_fp * spp;
        MTRY(ndwt_slab_segments_strided(to.plan, op, 1, d, sr, &cnt, mp->nrep, &ds, &ss, st));
        return NDWT_OK;
    }
    if (op != NDWT_SEG_COPY) return mfail(NDWT_ERR_UNSUPPORTED, "internal: adds across devices without peer access are staged");
    for (long long q = 0; q < mp->nrep; ++q)
        MHIP(hipMemcpyPeerAsync(dst + (size_t)(q * dst_fp) * pb, to.device, src + (size_t)(q * src_fp) * pb, from.device, (size_t)planes * pb, st));
    return NDWT_OK;
}

// copy `count` planes starting at GLOBAL plane g (periodic) of a per-slab plane array into dst (dst_fp planes per frame) on slab `to`, on
// `to`'s stream st.  plane_ptr(slab, local plane) = the source address in frame 0 of that slab's array (n planes per frame).
template <class SrcFn>
static int copy_planes(ndwt_mplan* mp, Slab& to, char* dst, long long dst_fp, long long g, long long count, SrcFn plane_ptr, hipStream_t st) {
    return walk(mp, g, count, [&](size_t o, long long lp, long long done, long long run) -> int {
        Slab& src = mp->slabs[o];
        return move_planes(mp, to, dst + (size_t)done * mp->plane_bytes, dst_fp, src, plane_ptr(src, lp), src.n, run, NDWT_SEG_COPY, st);
    });
}

// The level barrier between slabs (events only, the host does not block): every stream waits for ready[k] of the slabs within halo reach of
// its own -- the slabs whose approximation planes its next level copies (read after write) and whose copies read the buffer its level after
// next overwrites (write after read).  Slabs further away are ordered through those (a slab records ready[k] behind its waits of the level
// before).  With all G slabs waiting for all G (2 G^2 calls per level) this function was two thirds of the calls of a transform on 8 devices.
// Two phases: every slab's ready[k] is recorded (by the host) before any stream is told to wait for it.
static int barrier_record(ndwt_mplan* mp, size_t i, int k) {
    Slab& s = mp->slabs[i];
    MHIP(hipSetDevice(s.device));
    MHIP(hipEventRecord(s.ready[k], s.stream));
    return NDWT_OK;
}
static int barrier_wait(ndwt_mplan* mp, size_t i, int k) {
    Slab& s = mp->slabs[i];
    MHIP(hipSetDevice(s.device));
    for (int j : mp->nbr[i]) {
        Slab& o = mp->slabs[(size_t)j];
        if (&o != &s) MHIP(hipStreamWaitEvent(s.stream, o.ready[k], 0));
        MHIP(hipStreamWaitEvent(s.cstream, o.ready[k], 0));   // (its own slab's too: the copy stream is ordered by events only)
    }
    return NDWT_OK;
}
static int level_barrier(ndwt_mplan* mp, int k) {
    MRET(phase(mp, [&](size_t i) { return barrier_record(mp, i, k); }));
    return phase(mp, [&](size_t i) { return barrier_wait(mp, i, k); });
}

static int sync_all(ndwt_mplan* mp) {
    for (auto& s : mp->slabs) {
        MHIP(hipSetDevice(s.device));
        MHIP(hipStreamSynchronize(s.stream));
        MHIP(hipStreamSynchronize(s.cstream));
    }
    return NDWT_OK;
}

// the overlapped schedules cut a slab into the planes that need no neighbour and the rest: every slab must be thick enough for that
// (z-slabs have no run-of-planes entry points: the overlapped schedule is not offered)
static bool can_overlap(const ndwt_mplan* mp, long long before, long long after) {
    if (!mp->overlap || !mp->fast || z_slabs(mp)) return false;
    const long long m = before > after ? before : after;
    for (auto& s : mp->slabs)
        if (s.n < 2 * m + 1 || s.n <= before + after) return false;
    return true;
}

static int lazy_alloc(Slab& s, char** p, size_t bytes) {
    if (*p) return NDWT_OK;
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = hipMalloc((void**)p, bytes);
    if (e != hipSuccess) return mfail(NDWT_ERR_ALLOC, "device %d: hipMalloc(%zu bytes) failed: %s", s.device, bytes, hipGetErrorString(e));
    return NDWT_OK;
}

static int mcheck(const ndwt_mplan* mp, int level) {
    if (!mp) return mfail(NDWT_ERR_INVALID_ARG, "null plan");
    if (level < 1 || level > mp->max_level) return mfail(NDWT_ERR_INVALID_ARG, "level %d outside 1..max_level=%d of this plan", level, mp->max_level);
    return NDWT_OK;
}

// Both level loops serve both kinds of slab.  A slab of the outermost axis is one frame (R = 1) and its approximation buffers are
// [halo_max | n | halo_max] planes: the slab sits behind a margin of H = halo_max planes that takes the neighbours' planes in line.  A z-slab
// of a 4-D volume holds all nt frames of its planes, (nt, n, ny, nx) per band: a plane index of the sharded axis is R = nrep = nt runs of
// plane_bytes, frame q of a slab's array at q * n planes, and its buffers carry no margin (H = 0; the halo planes travel in hb / ha).

// ------------------------------------------------------------------------------------------------ analysis
// x[i]: the slab of the signal on slab i's device (n_i planes); y[i]: its coefficient slab, band b at b * n_i planes.  Queues the
// whole transform on the slabs' streams; the caller synchronises.
enum class DecStep {
    Overlapped,   // halo planes on the copy stream while the planes that need none of them are computed, then the two ends
    SplitHalo,    // halo planes into hb / ha, the slab read where it lies (z-slabs: every level; outermost axis: the caller's x at level 1)
    InlineHalo    // halo planes into the margins of the approximation buffer, in line with the slab
};

static int mdec_core(ndwt_mplan* mp, const void* const* x, void* const* y, int level) {
    const size_t pb = mp->plane_bytes;
    const long long R = mp->nrep, H = z_slabs(mp) ? 0 : mp->halo_max;
    const int nb = mp->nb;
    for (int lev = 1; lev <= level; ++lev) {
        const long long st = stride_of(mp, lev);
        const long long ab = (long long)(mp->L_outer / 2 - 1) * st, aa = (long long)(mp->L_outer / 2) * st, m = ab > aa ? ab : aa;
        // level lev reads approx[rd] (level 1: the caller's x) and writes its approximation into approx[wr] (the last level: band 0 of y)
        const int rd = ((lev - 1) & 1) ^ 1, wr = (lev - 1) & 1;
        const DecStep step = z_slabs(mp)                      ? DecStep::SplitHalo
                             : st == 1 && can_overlap(mp, ab, aa) ? DecStep::Overlapped
                             : lev == 1 && mp->fast && st == 1    ? DecStep::SplitHalo
                                                                  : DecStep::InlineHalo;
        // the level's input on a slab, and the source of its halo planes: the neighbours' inputs (produced in place by level lev - 1;
        // the producers were waited for at the end of that level)
        auto input = [&](Slab& o) -> const char* { return lev == 1 ? (const char*)x[index_of(mp, o)] : o.approx[rd] + (size_t)H * pb; };
        auto src = [&](Slab& o, long long lp) -> const char* { return input(o) + (size_t)lp * pb; };
        // one slab's work of this level (its copies out of the neighbours' buffers, its launches) and the record of its ready[wr]
        auto body = [&](size_t i) -> int {
            Slab& s = mp->slabs[i];
            MHIP(hipSetDevice(s.device));
            void* outs[16];
            outs[0] = lev == level ? y[i] : (void*)(s.approx[wr] + (size_t)H * pb);
            for (int b = 1; b < nb; ++b) outs[b] = (char*)y[i] + (size_t)(band_index(mp, level, lev, b) * R * s.n) * pb;
            const char* in = input(s);
            char* mid = s.approx[rd] + (size_t)H * pb;         // the margins before and after it take the neighbours' planes
            switch (step) {
            case DecStep::Overlapped: {
                // the caller's x has no margins around it: its halo planes go to hb / ha
                char* hb = lev == 1 ? s.hb : mid - (size_t)ab * pb;
                char* ha = lev == 1 ? s.ha : mid + (size_t)s.n * pb;
                void* oi[16];
                for (int b = 0; b < nb; ++b) oi[b] = (char*)outs[b] + (size_t)ab * pb;
                MRET(copy_planes(mp, s, hb, ab, s.z0 - ab, ab, src, s.cstream));
                MRET(copy_planes(mp, s, ha, aa, s.z0 + s.n, aa, src, s.cstream));
                MHIP(hipEventRecord(s.copied, s.cstream));
                MTRY(ndwt_analysis_level_slab_part(s.plan, in + (size_t)ab * pb, ab ? in : nullptr, in + (size_t)(s.n - aa) * pb, oi, 1, s.n - ab - aa, s.stream));
                MHIP(hipStreamWaitEvent(s.stream, s.copied, 0));
                if (lev == 1) {                               // the ends are two launches, halo planes from hb / ha
                    MTRY(ndwt_analysis_level_slab_part(s.plan, in, ab ? s.hb : nullptr, in + (size_t)m * pb, outs, 1, m, s.stream));
                    void* oe[16];
                    for (int b = 0; b < nb; ++b) oe[b] = (char*)outs[b] + (size_t)(s.n - m) * pb;
                    MTRY(ndwt_analysis_level_slab_part(s.plan, in + (size_t)(s.n - m) * pb, ab ? in + (size_t)(s.n - m - ab) * pb : nullptr, s.ha, oe, 1, m, s.stream));
                } else {
                    MTRY(ndwt_analysis_level_slab_runs(s.plan, mid - (size_t)ab * pb, outs, 1, m, 2, s.n - m, s.stream));   // both ends, one launch
                }
                break;
            }
            case DecStep::SplitHalo:
                MRET(copy_planes(mp, s, s.hb, ab, s.z0 - ab, ab, src, s.stream));
                MRET(copy_planes(mp, s, s.ha, aa, s.z0 + s.n, aa, src, s.stream));
                MTRY(ndwt_analysis_level_slab_split(s.plan, in, ab ? s.hb : nullptr, s.ha, outs, (int)st, s.stream));
                break;
            case DecStep::InlineHalo:
                if (lev == 1) {                               // kernels that want the halo planes in line with the slab: one copy of the slab of x
                    MRET(copy_planes(mp, s, mid - (size_t)ab * pb, 0, s.z0 - ab, ab + s.n + aa, src, s.stream));
                } else {
                    MRET(copy_planes(mp, s, mid - (size_t)ab * pb, 0, s.z0 - ab, ab, src, s.stream));
                    MRET(copy_planes(mp, s, mid + (size_t)s.n * pb, 0, s.z0 + s.n, aa, src, s.stream));
                }
                MTRY(ndwt_analysis_level_slab(s.plan, mid - (size_t)ab * pb, outs, (int)st, s.stream));
                break;
            }
            return barrier_record(mp, i, wr);
        };
        MRET(phase(mp, body));
        // approx[wr] of every slab is complete, and approx[rd] free to be overwritten by level lev + 1, once every slab's work of this
        // level (its launch and its halo copies out of the neighbours' buffers) is done: the level barrier's waits
        MRET(phase(mp, [&](size_t i) { return barrier_wait(mp, i, wr); }));
    }
    return NDWT_OK;
}

// ----------------------------------------------------------------------------------------------- synthesis
// partial sums of `count` planes starting at global plane g (periodic), held in `buf` on slab `from` (src_fp planes per frame): to their
// owners, added there.  dst_of(slab) = where that slab's n planes of this level's result live.
template <class DstFn>
static int scatter_margin(ndwt_mplan* mp, Slab& from, const char* buf, long long src_fp, long long g, long long count, DstFn dst_of) {
    const size_t pb = mp->plane_bytes;
    return walk(mp, g, count, [&](size_t o, long long lp, long long done, long long run) -> int {
        Slab& to = mp->slabs[o];
        MHIP(hipSetDevice(to.device));
        if (&to != &from) MHIP(hipStreamWaitEvent(to.stream, from.margins, 0));
        const char* src = buf + (size_t)done * pb;
        char* dst = dst_of(to) + (size_t)lp * pb;
        // add straight from the producer's buffer where the adding kernel can read it: the same memory, or (the segment kernel of z-slabs) a peer's
        if (mp->nrep > 1 ? direct_access(mp, to.device, from.device) : to.device == from.device)
            return move_planes(mp, to, dst, to.n, from, src, src_fp, run, NDWT_SEG_ADD, to.stream);
        MRET(move_planes(mp, to, to.recv, run, from, src, src_fp, run, NDWT_SEG_COPY, to.stream));   // staged: into the receive buffer, added from there
        return move_planes(mp, to, dst, to.n, to, to.recv, run, run, NDWT_SEG_ADD, to.stream);
    });
}

enum class RecStep {
    OverlappedScatter,   // the margins first, travelling on the destinations' copy streams while every slab synthesises its own planes
    ScatterParts,        // zero-extended synthesis in three parts: the slab's own planes in place, the margins into mb / ma
    ScatterExt,          // z-slabs: zero-extended synthesis into the slab's scratch, its own planes copied out
    Gather               // the halo planes of all bands assembled with the slab in the scratch
};

static int mrec_core(ndwt_mplan* mp, const void* const* y, void* const* x, int level) {
    const size_t pb = mp->plane_bytes;
    const long long R = mp->nrep, H = z_slabs(mp) ? 0 : mp->halo_max;
    const int nb = mp->nb;
    const long long smax = mp->dilation == NDWT_DILATION_ATROUS ? (1LL << (mp->max_level - 1)) : 1LL;
    for (int ind = 1; ind <= level; ++ind) {
        const int lev = level - ind + 1;
        const long long st = stride_of(mp, lev);
        const long long sb = (long long)(mp->L_outer / 2) * st, sa = (long long)(mp->L_outer / 2 - 1) * st, m = sa > sb ? sa : sb;
        const int rd = ind & 1, wr = rd ^ 1;             // level index ind > 1 reads the approximation level ind - 1 wrote into approx[rd]
        const bool scatter = mp->exchange == NDWT_EXCHANGE_SCATTER && mp->fast && st == 1;
        const RecStep step = !scatter                 ? RecStep::Gather
                             : z_slabs(mp)            ? RecStep::ScatterExt
                             : can_overlap(mp, sa, sb) ? RecStep::OverlappedScatter
                                                       : RecStep::ScatterParts;
        auto band_ptr = [&](Slab& o, int b) -> const char* {
            const char* yo = (const char*)y[index_of(mp, o)];
            if (b == 0) return ind == 1 ? yo : o.approx[rd] + (size_t)H * pb;
            return yo + (size_t)(band_index(mp, level, lev, b) * R * o.n) * pb;
        };
        auto dst_of = [&](Slab& o) -> char* { return lev == 1 ? (char*)x[index_of(mp, o)] : o.approx[wr] + (size_t)H * pb; };
        // the scratch of a slab: 2^d bands of its planes with their halo planes (z-slabs: their zero-extended result too), allocated on first use
        if (step == RecStep::Gather || step == RecStep::ScatterExt)
            for (auto& s : mp->slabs) MRET(lazy_alloc(s, &s.gather, (size_t)((long long)nb * R * (s.n + (long long)(mp->L_outer - 1) * smax)) * pb));
        switch (step) {
        case RecStep::OverlappedScatter:
            // margins first (one launch: two runs of m planes at the ends of the zero-extended result), so that they travel -- on the
            // destinations' copy streams -- while every slab synthesises its own planes; the adds follow that launch in stream order
            MRET(phase(mp, [&](size_t i) -> int {
                Slab& s = mp->slabs[i];
                MHIP(hipSetDevice(s.device));
                const void* ins[16];
                for (int b = 0; b < nb; ++b) ins[b] = band_ptr(s, b);
                MTRY(ndwt_synthesis_level_slab_runs(s.plan, ins, s.n, 0, s.n + sa + sb - m, 2, m, s.mb, 1, s.stream));   // mb: [run 0 | run 1]
                MHIP(hipEventRecord(s.margins, s.stream));
                MTRY(ndwt_synthesis_level_slab_part(s.plan, ins, s.n, sa, s.n, dst_of(s), 1, s.stream));
                return NDWT_OK;
            }));
            // the partial sums: run 0 holds planes [0, m) of the zero-extended result (the first sa: owed to the planes before the slab),
            // run 1 planes [n + sa + sb - m, n + sa + sb) (the last sb: the planes after it).  Copies to other devices go to the
            // destination's copy stream and a region of its receive buffer of their own; the adds come in slab order of the producers,
            // "before" margins first, behind the destination's own launch: the same fixed order of summation as without overlap.
            // Every DESTINATION slab queues what arrives at it (its own streams only): the producers' margins events were recorded in the
            // phase above.  The record of its ready[wr] (level barrier) closes the phase.
            MRET(phase(mp, [&](size_t ti) -> int {
                Slab& t = mp->slabs[ti];
                MHIP(hipSetDevice(t.device));
                struct Pending { char* dst; const char* src; long long run; };
                std::vector<Pending> adds;
                t.recv_used = 0;
                for (auto& from : mp->slabs) {
                    for (int side = 0; side < 2; ++side) {
                        const char* buf = side == 0 ? from.mb : from.mb + (size_t)(m + (m - sb)) * pb;
                        MRET(walk(mp, side == 0 ? from.z0 - sa : from.z0 + from.n, side == 0 ? sa : sb,
                                  [&](size_t o, long long lp, long long done, long long run) -> int {
                            if (o != ti) return NDWT_OK;
                            const char* src = buf + (size_t)done * pb;
                            char* dst = dst_of(t) + (size_t)lp * pb;
                            if (t.device != from.device || mp->overlap == 2) {   // (2: test hook -- the staged path between slabs of one device)
                                if (t.recv_used + run > 2 * mp->halo_max) return mfail(NDWT_ERR_UNSUPPORTED, "internal: receive buffer of the overlapped synthesis exhausted");
                                char* rb = t.recv + (size_t)t.recv_used * pb;
                                t.recv_used += run;
                                MHIP(hipStreamWaitEvent(t.cstream, from.margins, 0));
                                MRET(move_planes(mp, t, rb, run, from, src, run, run, NDWT_SEG_COPY, t.cstream));
                                src = rb;
                            } else if (&t != &from) {
                                MHIP(hipStreamWaitEvent(t.stream, from.margins, 0));   // same memory: added straight from the producer's buffer
                            }
                            adds.push_back({dst, src, run});
                            return NDWT_OK;
                        }));
                    }
                }
                MHIP(hipEventRecord(t.copied, t.cstream));
                MHIP(hipStreamWaitEvent(t.stream, t.copied, 0));
                for (auto& a : adds) MRET(move_planes(mp, t, a.dst, t.n, t, a.src, a.run, a.run, NDWT_SEG_ADD, t.stream));
                return barrier_record(mp, ti, wr);
            }));
            MRET(phase(mp, [&](size_t i) { return barrier_wait(mp, i, wr); }));
            continue;
        case RecStep::ScatterParts:
        case RecStep::ScatterExt:
            // zero-extended synthesis: plane k of the extended result = global plane z0 - sa + k.  The slab's own n planes go where
            // the result lives; the sa planes before and the sb planes after it are partial sums owed to their owners.
            for (auto& s : mp->slabs) {
                MHIP(hipSetDevice(s.device));
                const void* ins[16];
                for (int b = 0; b < nb; ++b) ins[b] = band_ptr(s, b);
                if (step == RecStep::ScatterExt) {            // the whole extended result in the scratch, (nt, sa + n + sb) planes
                    MTRY(ndwt_synthesis_level_slab_ext(s.plan, ins, s.gather, 1, s.stream));
                    MRET(move_planes(mp, s, dst_of(s), s.n, s, s.gather + (size_t)sa * pb, s.n + sa + sb, s.n, NDWT_SEG_COPY, s.stream));
                } else {
                    MTRY(ndwt_synthesis_level_slab_part(s.plan, ins, s.n, sa, s.n, dst_of(s), 1, s.stream));
                    if (sa) MTRY(ndwt_synthesis_level_slab_part(s.plan, ins, s.n, 0, sa, s.mb, 1, s.stream));
                    MTRY(ndwt_synthesis_level_slab_part(s.plan, ins, s.n, sa + s.n, sb, s.ma, 1, s.stream));
                }
                MHIP(hipEventRecord(s.margins, s.stream));
            }
            // a destination's own planes are written by its own stream before anything is added to them (stream order); the addends
            // arrive in slab order, "before" margins first: a fixed order of summation
            for (auto& s : mp->slabs) {
                const bool ext = step == RecStep::ScatterExt;
                MRET(scatter_margin(mp, s, ext ? s.gather : s.mb, s.n + sa + sb, s.z0 - sa, sa, dst_of));
                MRET(scatter_margin(mp, s, ext ? s.gather + (size_t)(sa + s.n) * pb : s.ma, s.n + sa + sb, s.z0 + s.n, sb, dst_of));
            }
            break;
        case RecStep::Gather:
            for (auto& s : mp->slabs) {
                MHIP(hipSetDevice(s.device));
                const long long nh = s.n + sb + sa;
                const void* ins[16];
                for (int b = 0; b < nb; ++b) {
                    char* dst = s.gather + (size_t)((long long)b * R * nh) * pb;
                    ins[b] = dst;
                    auto src = [&, b](Slab& o, long long lp) -> const char* { return band_ptr(o, b) + (size_t)lp * pb; };
                    MRET(copy_planes(mp, s, dst, nh, s.z0 - sb, nh, src, s.stream));   // all producers were waited for at the end of the previous level
                }
                MTRY(ndwt_synthesis_level_slab(s.plan, ins, dst_of(s), (int)st, s.stream));
            }
            break;
        }
        MRET(level_barrier(mp, wr));
    }
    return NDWT_OK;
}

extern "C" {

int ndwt_mplan_create(ndwt_mplan** out, int ndim, const int64_t* dims, const char* const* wnames, int dtype, int complexity,
                      int pres_l2_norm, int dilation, int max_level, const int* devices, int ndev) {
    return ndwt_mplan_create_axis(out, ndim, dims, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, devices, ndev, ndim - 1);
}

int ndwt_mplan_create_axis(ndwt_mplan** out, int ndim, const int64_t* dims, const char* const* wnames, int dtype, int complexity,
                           int pres_l2_norm, int dilation, int max_level, const int* devices, int ndev, int shard_axis) {
    if (!out) return mfail(NDWT_ERR_INVALID_ARG, "null plan pointer");
    *out = nullptr;
    if (ndim < 2 || ndim > NDWT_MAX_DIMS || !dims || !wnames || !devices || ndev < 1)
        return mfail(NDWT_ERR_INVALID_ARG, "multi-device plans shard the outermost of 2..4 axes over ndev >= 1 devices");
    if (shard_axis != ndim - 1 && !(ndim == 4 && shard_axis == 2))
        return mfail(NDWT_ERR_UNSUPPORTED, "shard_axis %d of a %d-D volume: multi-device plans shard the outermost axis (%d), or z (2) of a 4-D volume",
                     shard_axis, ndim, ndim - 1);
    const long long N = dims[shard_axis];
    if (ndev > N) return mfail(NDWT_ERR_INVALID_ARG, "more slabs (%d) than planes (%lld)", ndev, N);
    if (max_level < 1) return mfail(NDWT_ERR_INVALID_ARG, "max_level must be >= 1");
    ndwt_mplan* mp = new ndwt_mplan();
    mp->ndim = ndim; mp->dtype = dtype; mp->complexity = complexity; mp->max_level = max_level; mp->nb = 1 << ndim;
    mp->dilation = dilation;
    mp->exchange = NDWT_EXCHANGE_SCATTER;
    mp->overlap = 1;
    mp->threads = 1;
    mp->team = nullptr;
    for (int a = 0; a < ndim; ++a) mp->dims[a] = dims[a];
    mp->shard = shard_axis;
    mp->nrep = 1;
    for (int a = shard_axis + 1; a < ndim; ++a) mp->nrep *= dims[a];
    size_t pb = (dtype == NDWT_F32 ? 4 : 8) * (complexity == NDWT_COMPLEX_INTERLEAVED ? 2 : 1);
    for (int a = 0; a < shard_axis; ++a) pb *= (size_t)dims[a];
    mp->plane_bytes = pb;
    const size_t R = (size_t)mp->nrep;
    double lo[NDWT_MAX_TAPS], hi[NDWT_MAX_TAPS];
    int L = 0;
    if (ndwt_wave_filters(wnames[shard_axis], lo, hi, &L) != NDWT_OK) { delete mp; return mfail(NDWT_ERR_UNKNOWN_WAVELET, "Unknown Wavelet Name"); }
    mp->L_outer = L;
    const long long smax = dilation == NDWT_DILATION_ATROUS ? (1LL << (max_level - 1)) : 1LL;
    mp->halo_max = (long long)(L / 2) * smax;
    std::vector<int64_t> ld(dims, dims + ndim);
    const std::vector<ndwt::SlabPart> parts = ndwt::slab_partition(N, ndev);
    for (int i = 0; i < ndev; ++i) {
        Slab s;
        memset(&s, 0, sizeof s);
        s.device = devices[i];
        s.z0 = parts[(size_t)i].z0;
        s.n = parts[(size_t)i].n;
        mp->slabs.push_back(s);
    }
    for (size_t i = 0; i < mp->slabs.size(); ++i) mp->nbr.push_back(ndwt::slab_neighbours(mp->slabs, N, i, mp->halo_max));
    int rc = NDWT_OK;
    mp->fast = 1;
    for (auto& s : mp->slabs) {
        ld[shard_axis] = s.n;
        if ((rc = ndwt_plan_create_slab_axis(&s.plan, ndim, ld.data(), shard_axis, N, wnames, dtype, complexity, pres_l2_norm, dilation, 1, s.device)) != NDWT_OK) break;
        if (!ndwt_plan_slab_fast(s.plan)) mp->fast = 0;
        hipError_t e = hipSetDevice(s.device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.cstream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.copied, hipEventDisableTiming);
        for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&s.ready[k], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.margins, hipEventDisableTiming);
        // (R = frames of a z-slab: every buffer holds R runs of its planes; 1 for slabs of the outermost axis)
        for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipMalloc((void**)&s.approx[k], R * (size_t)(s.n + 2 * mp->halo_max) * pb);
        for (char** p : {&s.hb, &s.ha, &s.ma})
            if (e == hipSuccess) e = hipMalloc((void**)p, R * (size_t)mp->halo_max * pb);
        for (char** p : {&s.mb, &s.recv})               // mb: both margins of the overlapped synthesis (two runs); recv: a region per sender
            if (e == hipSuccess) e = hipMalloc((void**)p, R * (size_t)(2 * mp->halo_max) * pb);
        if (e != hipSuccess) { rc = mfail(NDWT_ERR_ALLOC, "device %d: %s", s.device, hipGetErrorString(e)); break; }
        for (auto& o : mp->slabs)                        // peer access where the runtime offers it (same-device pairs need none)
            if (o.device != s.device) {
                int can = 0;
                hipError_t pe = hipDeviceCanAccessPeer(&can, s.device, o.device);
                if (pe == hipSuccess && can) {
                    pe = hipDeviceEnablePeerAccess(o.device, 0);
                    if (pe == hipErrorPeerAccessAlreadyEnabled) pe = hipSuccess;
                    if (pe == hipSuccess) mp->peer.emplace_back(s.device, o.device);
                }
                (void)hipGetLastError();
                if (pe != hipSuccess || !can) {           // the copies still work (staged by the runtime), slower: say so
                    char note[160];
                    snprintf(note, sizeof note, "no peer access %d -> %d (%s); ", s.device, o.device, pe != hipSuccess ? hipGetErrorString(pe) : "not offered");
                    if (mp->notes.find(note) == std::string::npos) mp->notes += note;
                }
            }
    }
    if (rc != NDWT_OK) {
        std::string keep = rc == NDWT_ERR_ALLOC ? g_merr : std::string(ndwt_last_error());
        ndwt_mplan_destroy(mp);
        return mfail(rc, "%s", keep.c_str());
    }
    *out = mp;
    return NDWT_OK;
}

int ndwt_mplan_destroy(ndwt_mplan* mp) {
    if (!mp) return NDWT_OK;
    team_destroy(mp);
    for (auto& s : mp->slabs) {
        (void)hipSetDevice(s.device);
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.plan) ndwt_plan_destroy(s.plan);
        for (int k = 0; k < 2; ++k) {
            if (s.approx[k]) (void)hipFree(s.approx[k]);
            if (s.ready[k]) (void)hipEventDestroy(s.ready[k]);
        }
        if (s.margins) (void)hipEventDestroy(s.margins);
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.cstream) { (void)hipStreamSynchronize(s.cstream); (void)hipStreamDestroy(s.cstream); }
        for (char* p : {s.hb, s.ha, s.mb, s.ma, s.recv, s.gather, s.xbuf, s.coef})
            if (p) (void)hipFree(p);
        if (s.stream) (void)hipStreamDestroy(s.stream);
    }
    delete mp;
    return NDWT_OK;
}

int ndwt_mplan_num_slabs(const ndwt_mplan* mp) { return mp ? (int)mp->slabs.size() : -1; }

int ndwt_mplan_slab(const ndwt_mplan* mp, int idx, int* device, int64_t* first_plane, int64_t* planes) {
    if (!mp || idx < 0 || idx >= (int)mp->slabs.size()) return mfail(NDWT_ERR_INVALID_ARG, "bad slab index");
    if (device) *device = mp->slabs[idx].device;
    if (first_plane) *first_plane = mp->slabs[idx].z0;
    if (planes) *planes = mp->slabs[idx].n;
    return NDWT_OK;
}

int ndwt_mplan_set_exchange(ndwt_mplan* mp, int exchange) {
    if (!mp || (exchange != NDWT_EXCHANGE_SCATTER && exchange != NDWT_EXCHANGE_GATHER)) return mfail(NDWT_ERR_INVALID_ARG, "bad plan / exchange scheme");
    mp->exchange = exchange;
    return NDWT_OK;
}

int ndwt_mplan_set_overlap(ndwt_mplan* mp, int overlap) {
    if (!mp) return mfail(NDWT_ERR_INVALID_ARG, "null plan");
    mp->overlap = overlap == 2 ? 2 : (overlap ? 1 : 0);
    return NDWT_OK;
}

int ndwt_mplan_set_threads(ndwt_mplan* mp, int threads) {
    if (!mp) return mfail(NDWT_ERR_INVALID_ARG, "null plan");
    mp->threads = threads ? 1 : 0;
    if (!mp->threads) team_destroy(mp);
    return NDWT_OK;
}

double ndwt_mplan_last_enqueue_us(const ndwt_mplan* mp) { return mp ? mp->last_enqueue_us : -1.0; }

int ndwt_mplan_describe(const ndwt_mplan* mp, char* buf, int buflen) {
    if (!mp || !buf || buflen < 1) return mfail(NDWT_ERR_INVALID_ARG, "bad arguments");
    const bool scatter = mp->exchange == NDWT_EXCHANGE_SCATTER && mp->fast && mp->dilation == NDWT_DILATION_REFERENCE;
    const bool z = mp->shard != mp->ndim - 1;
    snprintf(buf, (size_t)buflen, "%d slabs of axis %d (%s); analysis: halo planes of the approximation band%s; synthesis: %s; %s; %s", (int)mp->slabs.size(),
             mp->shard, z ? "z, t whole on every slab" : "outermost", (mp->fast && !z) ? ", slabs read in place" : "",
             scatter ? "scatter-add of one band of partial sums" : "gather of the halo planes of all bands",
             (mp->overlap && mp->fast && !z) ? "exchange overlapped with the planes that do not wait for it (where every slab is thick enough)" : "exchange, then compute",
             mp->notes.empty() ? "peer access between all devices" : mp->notes.c_str());
    return NDWT_OK;
}

typedef int (*CoreFn)(ndwt_mplan*, const void* const*, void* const*, int);   // mdec_core / mrec_core: (plan, slabs in, slabs out, level)

// device-resident form: x_slabs[i] / y_slabs[i] live on slab i's device (ndwt_mplan_slab: n_i planes of x; band b of the coefficient
// slab at b * n_i planes).  The data must be complete when the call is made (no stream of the caller is waited for); the call returns
// when the result is.
static int run_slabs(ndwt_mplan* mp, CoreFn core, const void* const* in, void* const* out, int level) {
    int rc = mcheck(mp, level);
    if (rc) return rc;
    if (!in || !out) return mfail(NDWT_ERR_INVALID_ARG, "null pointer array");
    for (size_t i = 0; i < mp->slabs.size(); ++i)
        if (!in[i] || !out[i]) return mfail(NDWT_ERR_INVALID_ARG, "null slab pointer %zu", i);
    const auto t0 = std::chrono::steady_clock::now();
    team_begin(mp);
    rc = core(mp, in, out, level);
    team_end(mp);
    mp->last_enqueue_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    const int rs = sync_all(mp);                          // (also after an error: nothing stays queued on buffers the caller owns)
    return rc ? rc : rs;
}

int ndwt_mdec(ndwt_mplan* mp, const void* const* x_slabs, void* const* y_slabs, int level) { return run_slabs(mp, mdec_core, x_slabs, y_slabs, level); }

int ndwt_mrec(ndwt_mplan* mp, const void* const* y_slabs, void* const* x_slabs, int level) { return run_slabs(mp, mrec_core, y_slabs, x_slabs, level); }

// whole-volume host arrays in, whole-volume host arrays out (the layout the MATLAB gateway holds): x is prod(dims) elements,
// y prod(dims) * ndwt_num_bands(ndim, level), band-planar.  Blocks until the result is in y.
static int host_buffers(ndwt_mplan* mp, std::vector<void*>& xs, std::vector<void*>& ys) {
    const long long nbt = (long long)ndwt_num_bands(mp->ndim, mp->max_level);
    for (auto& s : mp->slabs) {
        MRET(lazy_alloc(s, &s.xbuf, (size_t)(mp->nrep * s.n) * mp->plane_bytes));
        MRET(lazy_alloc(s, &s.coef, (size_t)(nbt * mp->nrep * s.n) * mp->plane_bytes));
        xs.push_back(s.xbuf);
        ys.push_back(s.coef);
    }
    return NDWT_OK;
}

// slab i's share of a whole-volume host array to (to_device) or from its buffer `dev`, on the slab's stream.  The host array is `rows`
// planar arrays of the volume (1: x; the number of bands: coefficients), the buffer the same rows of the slab.
static int stage(ndwt_mplan* mp, size_t i, char* host, char* dev, long long rows, bool to_device) {
    Slab& s = mp->slabs[i];
    const size_t pb = mp->plane_bytes, run = (size_t)s.n * pb, pitch = (size_t)axis_len(mp) * pb;
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    MHIP(hipSetDevice(s.device));
    host += (size_t)s.z0 * pb;
    if (mp->nrep > 1) {
        // z-slab: a run of n planes from every frame of the volume (rows of N planes); row b, frame q is row b * nt + q on both sides
        if (to_device) MHIP(hipMemcpy2DAsync(dev, run, host, pitch, run, (size_t)(rows * mp->nrep), kind, s.stream));
        else MHIP(hipMemcpy2DAsync(host, pitch, dev, run, run, (size_t)(rows * mp->nrep), kind, s.stream));
        return NDWT_OK;
    }
    for (long long b = 0; b < rows; ++b) {
        if (to_device) MHIP(hipMemcpyAsync(dev + (size_t)b * run, host + (size_t)b * pitch, run, kind, s.stream));
        else MHIP(hipMemcpyAsync(host + (size_t)b * pitch, dev + (size_t)b * run, run, kind, s.stream));
    }
    return NDWT_OK;
}

// analysis: x_host -> xbuf, mdec_core, coef -> y_host; synthesis: y_host -> coef, mrec_core, xbuf -> x_host
static int run_host(ndwt_mplan* mp, bool analysis, const void* in_host, void* out_host, int level) {
    int rc = mcheck(mp, level);
    if (rc) return rc;
    if (!in_host || !out_host) return mfail(NDWT_ERR_INVALID_ARG, "null data pointer");
    const long long nbt = (long long)ndwt_num_bands(mp->ndim, level);
    std::vector<void*> xs, ys;
    MRET(host_buffers(mp, xs, ys));
    std::vector<void*>&in = analysis ? xs : ys, &out = analysis ? ys : xs;
    // the copies between the host arrays and the slabs are queued by the slabs' own threads too: from pageable memory (what MATLAB holds) a
    // copy occupies its calling thread until it is staged, and one thread would serve the devices' links one after the other
    team_begin(mp);
    rc = phase(mp, [&](size_t i) { return stage(mp, i, (char*)in_host, (char*)in[i], analysis ? 1 : nbt, true); });
    if (rc == NDWT_OK) rc = level_barrier(mp, 1);         // every slab of the input is in place before a neighbour reads its halo planes
    if (rc == NDWT_OK) rc = (analysis ? mdec_core : mrec_core)(mp, in.data(), out.data(), level);
    if (rc == NDWT_OK) rc = phase(mp, [&](size_t i) { return stage(mp, i, (char*)out_host, (char*)out[i], analysis ? nbt : 1, false); });
    team_end(mp);
    const int rs = sync_all(mp);
    return rc ? rc : rs;
}

int ndwt_mdec_host(ndwt_mplan* mp, const void* x_host, void* y_host, int level) { return run_host(mp, true, x_host, y_host, level); }

int ndwt_mrec_host(ndwt_mplan* mp, const void* y_host, void* x_host, int level) { return run_host(mp, false, y_host, x_host, level); }

const char* ndwt_mplan_last_error(void) { return g_merr.c_str(); }

}  // extern "C"
