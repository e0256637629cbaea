// ndwt_api.hip -- plan, level loop, axis kernels and the C ABI of libndwt_hip.so (include/ndwt.h).
//
// Replaces, for the hot path, reference mex/nddwt.c (nd_dwt_dec :189-239, nd_dwt_rec :242-292 and
// their 1-level forms :98-186) and the gateway mex/nd_dwt_mex.c:8-153.  No CPU fallback exists in
// this library: every entry point runs HIP kernels or returns an error code.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ndwt.h"
#include "ndwt_device.h"
#include "ndwt_device_items.h"
#include "ndwt_device_joint.h"
#include "ndwt_device_joint_tile.h"
#include "ndwt_device_neigh.h"
#include "ndwt_device_norms.h"
#include "ndwt_device_risk.h"
#include "ndwt_device_select.h"
#include "ndwt_filters.h"
#include "ndwt_fused.h"
#include "ndwt_geom.h"
#include "ndwt_select.h"
#include "ndwt_shrink.h"
#include "ndwt_taps_host.h"
#include "ndwt_trace.h"

using namespace ndwt;

// ------------------------------------------------------------------------------------------ errors
static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(NDWT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------------------------ launch trace
namespace ndwt {
std::atomic<int> g_trace_on{0};
static std::mutex g_trace_mu;
static std::string g_trace_log;
static constexpr size_t kTraceCap = 8u << 20;            // records past 8 MB are dropped (a test turns the trace on around a few calls)

void trace_append(const std::string& kernel, dim3 grid, dim3 block) {
    char geo[96];
    snprintf(geo, sizeof geo, " grid=(%u,%u,%u) block=(%u,%u,%u)\n", grid.x, grid.y, grid.z, block.x, block.y, block.z);
    std::lock_guard<std::mutex> lk(g_trace_mu);
    if (!g_trace_on.load(std::memory_order_relaxed) || g_trace_log.size() + kernel.size() + strlen(geo) > kTraceCap) return;
    g_trace_log += kernel;
    g_trace_log += geo;
}

void trace_append_pretty(const char* pretty, dim3 grid, dim3 block) {
    const char* b = strstr(pretty, "[K = ");
    const char* e = pretty + strlen(pretty);
    if (!b || e == pretty || e[-1] != ']') { trace_append(pretty, grid, block); return; }
    trace_append(std::string(b + 5, e - 1), grid, block);
}
}  // namespace ndwt

// ------------------------------------------------------------------------------------ axis kernels
template <typename T>
__global__ __launch_bounds__(256) void axis_analysis_kernel(const T* __restrict__ in, T* __restrict__ lo, T* __restrict__ hi,
                                                            const AxisTaps<T> tp, const AxisArgs<T> a) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (; idx < a.total; idx += step) axis_analysis_elem(idx, in, lo, hi, tp, a);
}

template <typename T>
__global__ __launch_bounds__(256) void axis_synthesis_kernel(const T* __restrict__ ain, const T* __restrict__ din,
                                                             T* __restrict__ out, const AxisTaps<T> tp, const AxisArgs<T> a) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (; idx < a.total; idx += step) axis_synthesis_elem(idx, ain, din, out, tp, a);
}

// -------------------------------------------------------------------------------------------- plan
struct ProfRec {
    int kind;                          // NDWT_KERNEL_*
    hipEvent_t start, stop;
};

#ifdef NDWT_NO_APPROX_SKEW
static constexpr size_t kApproxSkew = 0;
#else
static constexpr size_t kApproxSkew = 256;
#endif
// A device allocation owned by value: move-only, freed by its destructor (on the device that is current then).  It only ever grows, and
// growing does not keep the contents: every user fills the buffer before reading it.
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); return *this; }
    ~DevBuf() { reset(); }
    void reset() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    // at least `need` bytes.  Large enough: nothing happens.  Else the device is synchronised (work in flight may still read the old
    // block), the block freed and a new one allocated; on failure the buffer is empty.  what: "for temporaries", "of the staging buffer"
    int grow(size_t need, const char* what, bool say_bytes = true) {
        if (need <= bytes) return NDWT_OK;
        if (ptr) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipFree(ptr));
            ptr = nullptr;
            bytes = 0;
        }
        const hipError_t e = hipMalloc(&ptr, need);
        if (e != hipSuccess) {
            ptr = nullptr;
            return say_bytes ? fail(NDWT_ERR_ALLOC, "hipMalloc(%zu bytes) %s failed: %s", need, what, hipGetErrorString(e))
                             : fail(NDWT_ERR_ALLOC, "hipMalloc %s failed: %s", what, hipGetErrorString(e));
        }
        bytes = need;
        return NDWT_OK;
    }
    // a table the kernels read: allocated and filled from host memory (synchronously)
    int upload(const void* host, size_t n, const char* what) {
        reset();
        hipError_t e = hipMalloc(&ptr, n);
        if (e == hipSuccess) { bytes = n; e = hipMemcpy(ptr, host, n, hipMemcpyHostToDevice); }
        if (e == hipSuccess) return NDWT_OK;
        reset();
        return fail(NDWT_ERR_ALLOC, "uploading %s failed: %s", what, hipGetErrorString(e));
    }
};

struct ndwt_plan {
    int ndim = 0;
    long long dims[NDWT_MAX_DIMS] = {};
    int order[NDWT_MAX_DIMS] = {};     // K of dbK per axis
    AxisFilter filt[NDWT_MAX_DIMS] = {};
    int dtype = 0, complexity = 0, l2 = 0, dilation = 0, max_level = 0, device = 0, path = NDWT_PATH_AUTO;
    size_t esize = 0;                  // bytes per scalar
    long long comp = 1;                // scalars per element (2 for interleaved complex)
    long long vol = 0;                 // scalars per band (a batched plan: of all its signals / items)
    long long howmany = 0;             // ndwt_plan_create_many: signals of a batched 1-D plan, signal k at k * dims[0] elements; 0 = not batched.
                                       // ndwt_plan_create_axes: the items of a stack -- ndim and dims are those of ONE item (an image or a
                                       // volume), item j at j * item_vol() scalars of the input and of every band
    long long inner = 1;               // ndwt_plan_create_interleaved: elements of a sample that lie together, faster in memory than dims[0]
                                       // (the array is [inner, dims.., howmany]); 1 everywhere else
    DevBuf approx_base[2];             // approximation ping-pong between levels, each kApproxSkew bytes larger than a band: approx(i) is the band
    DevBuf tmp;                        // temporaries of the per-axis path / 4-D split
    int target_blocks = 0;             // fused-kernel grid sizing: 0 = one round of resident workgroups (per kernel), else as given
    int force_zchunk = 0;
    int zchunk_dir[2] = {0, 0};        // per-direction override of the marched chunk: [0] analysis, [1] synthesis (0 = auto)
    int variant_fwd = 0, variant_inv = 0;   // fused-kernel variants (tuning experiments; same results: ndwt_select.h)
    bool uniform_yz = false;           // the y and z axes carry the same synthesis taps: Inv3Y then keeps one set of tap pairs for both
    int num_cus = 0;
    int fp64_fused = 1;                // fp64: fused 3-D kernels (1) or the per-axis march kernels (0) -- measured: 256^3 fp64 db4 L3 2.5 ms
                                       // fused (LDS analysis + lane-shift synthesis) vs 4.1 ms per-axis
    DevBuf taps_dev[2];                // device tap tables of the fused kernels: [0] analysis (Taps3<T, Lp>), [1] synthesis (Taps3Y<T, Lp>)
    DevBuf coef;                       // coefficient scratch of ndwt_denoise (all bands of the last level used), lazily allocated
    DevBuf taps_den;                   // device tap table of the fused level-1 denoising kernel (TapsDen<float, L>), built at plan creation where it applies
    DevBuf select_buf;                 // ndwt_band_select: the device-side state and the global histogram (SelectState, then [slot][bin]); lazily allocated
    DevBuf norms_buf;                  // ndwt_band_norms*: the results of the host forms ([item][band][4] doubles), then the partials of the chunks
                                       // ([band][item][chunk][4]); lazily allocated, only ever grown
    double sigma_gain = 0.0;           // ndwt_estimate_sigma*: the gain of the last level-1 band (last_band_gain), computed at the first call
    // the threshold table of the *_items calls ([item][band], in the plan's scalar type): written into a pinned host buffer, copied to a
    // device buffer on the call's stream; both only grow.  thr_event is recorded behind the copy: the next call waits for it before it
    // overwrites the pinned buffer (the copy may still be reading it)
    DevBuf thr_dev;
    void* thr_host = nullptr;
    size_t thr_host_bytes = 0;
    hipEvent_t thr_event = nullptr;
    bool thr_copy_pending = false;
    DevBuf taps_den1;                  // a batched 1-D plan whose levels can cascade: Taps1D<T, L>, the tables of both directions for Den1C
    DevBuf den_a1;                     // ndwt_denoise, fused level 1: the level-1 approximation / its reconstruction -- a scratch of its own (lazily
                                       // allocated), not `tmp`: dec_impl / rec_impl run in between and may re-allocate that one
    int fused_level1 = 1;              // ndwt_denoise: 1 (default) level 1 in one launch where that is faster (tap lengths <= 6), 2 wherever the
                                       // kernel exists (8 taps too: compute-bound there, +3 %), 0 never (the level-1 detail bands stay in memory)
    // optional per-kernel timing with HIP events on the launch stream (bench.py's roofline figures); a launch records through the
    // const plan it is given
    int profiling = 0;
    mutable std::vector<ProfRec> prof;
    mutable std::vector<hipEvent_t> ev_pool;   // profiling events, reused
    long long* stamps = nullptr;       // diagnostic builds (-DNDWT_STAMPS): device buffer for the per-wave phase cycle sums
    DevBuf stage[2];                   // device staging of the host-pointer forms: [0] one band (x / the result), [1] all bands; lazily grown,
                                       // kept across calls (ndwt_plan_release_staging frees them)
    int live_coefs = 0;                // ndwt_coef handles bound to this plan
    int thin_slab = 0;                 // slab plan whose outer axis is shorter than its filter: slab entry points only
    int shard = 0;                     // slab plans: the sharded axis (ndim-1, or 2 for a 4-D volume sharded on z); halos live on it
    DevBuf zin;                        // z-slabs, split-halo analysis: the slab assembled with its halo planes (lazily allocated)

    // 256 B off the allocation's (power-of-two) alignment: the approximation is then the one band of a level that does not share the
    // address bits below 1 KiB with the packed detail bands (about a quarter of the pitched gain)
    void* approx(int i) const { return (char*)approx_base[i].ptr + kApproxSkew; }
    long long items() const { return howmany > 0 ? howmany : 1; }
    long long item_vol() const { return vol / items(); }   // scalars of one item of a band (an unbatched plan: the band)
    ~ndwt_plan() {                     // (the buffers free themselves; the caller has made the plan's device current)
        for (auto& r : prof) { (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop); }
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        if (thr_event) (void)hipEventDestroy(thr_event);
        if (thr_host) (void)hipHostFree(thr_host);
    }
};

// The plan's scalar type as a type: f is a generic lambda, called with a float or a double (only its type matters).
template <class F> static int with_scalar(const ndwt_plan* p, F&& f) { return p->dtype == NDWT_F32 ? f(float()) : f(double()); }
// What an entry point does once its arguments are checked: make the plan's device current, then run f for the plan's scalar type.
template <class F> static int on_device(const ndwt_plan* p, F&& f) {
    HIP_TRY(hipSetDevice(p->device));
    return with_scalar(p, f);
}

// Events come from a pool owned by the plan (get_profile returns them to it), and a launch that did not happen
// (rc != 0: a cascade that declined, whose caller takes one launch per level, or an error) leaves no record.
static bool prof_event(const ndwt_plan* p, hipEvent_t* e) {
    if (!p->ev_pool.empty()) { *e = p->ev_pool.back(); p->ev_pool.pop_back(); return true; }
    return hipEventCreate(e) == hipSuccess;
}
static void prof_begin(const ndwt_plan* p, int kind, hipStream_t s) {
    if (!p->profiling) return;
    ProfRec r;
    r.kind = kind;
    if (!prof_event(p, &r.start)) return;
    if (!prof_event(p, &r.stop)) { p->ev_pool.push_back(r.start); return; }
    (void)hipEventRecord(r.start, s);
    p->prof.push_back(r);
}
static void prof_end(const ndwt_plan* p, hipStream_t s, int rc = 0) {
    if (!p->profiling || p->prof.empty()) return;
    if (rc != 0) {                                        // nothing was launched: drop the record
        p->ev_pool.push_back(p->prof.back().start);
        p->ev_pool.push_back(p->prof.back().stop);
        p->prof.pop_back();
        return;
    }
    (void)hipEventRecord(p->prof.back().stop, s);
}

static long long level_stride(const ndwt_plan* p, int lev) { return p->dilation == NDWT_DILATION_ATROUS ? (1LL << (lev - 1)) : 1LL; }

template <typename T> static bool aligned_vec4(const void* ptr) { return ((uintptr_t)ptr % (4 * sizeof(T))) == 0; }

// ------------------------------------------------------------------------------ one axis, one pass
// The view [outer][n][inner] of the pass and whether its pointers lie on groups of 4 scalars go to axis_select (ndwt_select.h), which
// names the kernel and its launch geometry; this function launches what the pick names.
template <typename T>
static int axis_pass(const ndwt_plan* p, bool synthesis, int axis, const long long* dims_cur, long long stride, bool wrap,
                     const T* in0, const T* in1, T* out0, T* out1, hipStream_t s) {
    const AxisFilter& f = p->filt[axis];
    const double *lo = synthesis ? f.syn_lo : f.ana_lo, *hi = synthesis ? f.syn_hi : f.ana_hi;
    AxisArgs<T> a;
    a.inner = p->comp * p->inner;                         // (interleaved samples: axis 0 is strided too)
    for (int k = 0; k < axis; ++k) a.inner *= dims_cur[k];
    a.outer = p->howmany > 0 ? p->howmany : 1;            // (a batched 1-D plan: its signals are the rows)
    for (int k = axis + 1; k < p->ndim; ++k) a.outer *= dims_cur[k];
    a.n = dims_cur[axis];
    a.stride = stride;
    a.left = (synthesis ? (long long)(f.len / 2) : (long long)(f.len / 2 - 1)) * stride;
    a.wrap = wrap ? 1 : 0;
    a.n_in = wrap ? a.n : a.n + (long long)(f.len - 1) * stride;
    a.total = a.outer * a.n * a.inner;
    if (a.total == 0) return NDWT_OK;
    const bool aligned = aligned_vec4<T>(in0) && (!synthesis || aligned_vec4<T>(in1)) && aligned_vec4<T>(out0) && (synthesis || aligned_vec4<T>(out1));
    const AxisQuery q = {sizeof(T) == 8, synthesis, p->path == NDWT_PATH_AUTO, wrap, f.len, stride, (int)p->comp, a.inner, a.n, a.outer,
                         axis == 0 && p->inner == 1, aligned};
    const AxisPick k = axis_select(q);
    int rc;
    prof_begin(p, synthesis ? NDWT_KERNEL_AXIS_SYNTHESIS : NDWT_KERNEL_AXIS_ANALYSIS, s);
    if (k.kernel == kAxisMarch) {
        const MarchArgs<T> m = {in0, in1, out0, out1, k.inner, k.n, k.n_in, a.outer, k.chunk, k.nchunks, a.wrap, k.ngroups};
        rc = launch_axis_march(k.march(), m, lo, hi, s);
    } else if (k.kernel == kAxisX) {
        const AxisXArgs<T> x = {in0, in1, out0, out1, k.row, a.outer, k.nseg};
        rc = launch_axisx(k.axisx(), x, lo, hi, s);
    } else {
        AxisTaps<T> tp;
        tp.len = f.len;
        for (int j = 0; j < kMaxTaps; ++j) { tp.lo[j] = j < f.len ? (T)lo[j] : 0; tp.hi[j] = j < f.len ? (T)hi[j] : 0; }
        trace_plain(dim3((unsigned)k.grid), dim3(256), synthesis ? "axis_synthesis_kernel" : "axis_analysis_kernel", trace_scalar<T>());
        if (synthesis)
            hipLaunchKernelGGL(axis_synthesis_kernel<T>, dim3((unsigned)k.grid), dim3(256), 0, s, in0, in1, out0, tp, a);
        else
            hipLaunchKernelGGL(axis_analysis_kernel<T>, dim3((unsigned)k.grid), dim3(256), 0, s, in0, out0, out1, tp, a);
        rc = (int)hipGetLastError();
    }
    prof_end(p, s, rc);
    // (-1, -2: after a pick, internal errors -- see fused3_run)
    if (rc == -1) return fail(NDWT_ERR_UNSUPPORTED, "internal: no per-axis kernel instantiated for the pick (kernel %d, tap length %d)", (int)k.kernel, f.len);
    if (rc == -2) return fail(NDWT_ERR_UNSUPPORTED, "internal: launch geometry does not match the per-axis kernel's chunks or segments, or its grid is beyond 2^31 - 1");
    if (rc != 0) return fail(NDWT_ERR_HIP, "per-axis kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return NDWT_OK;
}

// ---------------------------------------------------------------------- per-axis (general) levels
// depth-first over the band tree, outermost axis first; temporaries: 2 volumes per tree depth
template <typename T> struct GenericCtx {
    const ndwt_plan* p;
    long long stride;
    bool slab;
    long long dims_cur[NDWT_MAX_DIMS];
    T* tmp;                  // 2*(ndim-1) volumes of vol_tmp scalars
    long long vol_tmp;
    hipStream_t s;
    long long n_in;          // slab mode: planes of the sharded axis p->shard with its halo (the local planes: dims_cur[p->shard])
};

// dims a pass on `axis` sees in slab mode: the sharded axis carries its halo planes until its own pass trims them (analysis: the
// passes of the axes above it run on the haloed slab; synthesis: the passes of the axes below it do).  Outer-axis slabs: every pass
// sees the local planes in the analysis (the outer pass is its first) and the haloed slab up to the last pass of the synthesis.
template <typename T> static const long long* generic_dims(const GenericCtx<T>& c, int axis, bool synthesis, long long* buf) {
    if (!c.slab) return c.dims_cur;
    for (int k = 0; k < c.p->ndim; ++k) buf[k] = c.dims_cur[k];
    if (synthesis ? axis < c.p->shard : axis > c.p->shard) buf[c.p->shard] = c.n_in;
    return buf;
}

template <typename T> static int generic_analysis(GenericCtx<T>& c, int axis, const T* src, int prefix, T* const* out) {
    const bool wrap = !(c.slab && axis == c.p->shard);
    long long dbuf[NDWT_MAX_DIMS];
    const long long* dims = generic_dims(c, axis, false, dbuf);
    if (axis == 0) return axis_pass<T>(c.p, false, 0, dims, c.stride, wrap, src, nullptr, out[prefix], out[prefix | 1], c.s);
    T* lo = c.tmp + (long long)(2 * (axis - 1)) * c.vol_tmp;
    T* hi = lo + c.vol_tmp;
    int rc = axis_pass<T>(c.p, false, axis, dims, c.stride, wrap, src, nullptr, lo, hi, c.s);
    if (rc) return rc;
    rc = generic_analysis(c, axis - 1, lo, prefix, out);
    if (rc) return rc;
    return generic_analysis(c, axis - 1, hi, prefix | (1 << axis), out);
}

template <typename T> static int generic_synthesis(GenericCtx<T>& c, int axis, int prefix, const T* const* in, T* dst) {
    const bool wrap = !(c.slab && axis == c.p->shard);
    long long dbuf[NDWT_MAX_DIMS];
    const long long* dims = generic_dims(c, axis, true, dbuf);
    if (axis == 0) return axis_pass<T>(c.p, true, 0, dims, c.stride, wrap, in[prefix], in[prefix | 1], dst, nullptr, c.s);
    T* a = c.tmp + (long long)(2 * (axis - 1)) * c.vol_tmp;
    T* d = a + c.vol_tmp;
    int rc = generic_synthesis(c, axis - 1, prefix, in, a);
    if (rc) return rc;
    rc = generic_synthesis(c, axis - 1, prefix | (1 << axis), in, d);
    if (rc) return rc;
    return axis_pass<T>(c.p, true, axis, dims, c.stride, wrap, a, d, dst, nullptr, c.s);
}

// one level by per-axis passes: in[0] -> the 2^d bands out[], or the 2^d bands in[] -> out[0]; slab: halo on the sharded axis p->shard
template <typename T> static int per_axis_level(ndwt_plan* p, bool synthesis, const T* const* in, T* const* out, long long stride, bool slab, hipStream_t s) {
    const int d = p->ndim, sh = p->shard;
    GenericCtx<T> c;
    c.p = p; c.stride = stride; c.slab = slab; c.s = s;
    for (int k = 0; k < d; ++k) c.dims_cur[k] = p->dims[k];
    c.n_in = p->dims[sh] + (slab ? (long long)(p->filt[sh].len - 1) * stride : 0);
    // the temporaries hold haloed slabs, except in the analysis of an outer-axis slab: its first pass trims the halo
    c.vol_tmp = (synthesis || sh != d - 1) ? p->vol / p->dims[sh] * c.n_in : p->vol;
    int rc = p->tmp.grow((size_t)(2 * (d - 1)) * (size_t)c.vol_tmp * sizeof(T), "for temporaries");
    if (rc) return rc;
    c.tmp = (T*)p->tmp.ptr;
    return synthesis ? generic_synthesis<T>(c, d - 1, 0, in, out[0]) : generic_analysis<T>(c, d - 1, in[0], 0, out);
}

// ------------------------------------------------------------------------------------ fused levels
// The eligibility predicates and the choice of kernel are plain functions of integers (ndwt_select.h); this is what they see of a plan.
static SelPlan sel(const ndwt_plan* p) {
    SelPlan q = {p->ndim, (int)p->comp, p->dtype == NDWT_F64, p->complexity == NDWT_REAL, p->path == NDWT_PATH_AUTO,
                 p->dilation != NDWT_DILATION_REFERENCE, p->fp64_fused != 0, {1, 1, 1, 1}, {2, 2, 2, 2}, p->variant_fwd, p->variant_inv, p->howmany, p->inner};
    for (int k = 0; k < p->ndim; ++k) { q.dims[k] = p->dims[k]; q.len[k] = p->filt[k].len; }
    return q;
}

static FusedTapsD fused_taps(const ndwt_plan* p, int Lp, bool synthesis) {
    FusedTapsD t;
    t.Lp = Lp;
    for (int a = 0; a < 3; ++a) {
        if (a >= p->ndim) {
            for (int j = 0; j < kMaxTaps; ++j) t.lo[a][j] = t.hi[a][j] = 0.0;
            continue;
        }
        const AxisFilter& f = p->filt[a];
        pad_taps(synthesis ? f.syn_lo : f.ana_lo, f.len, Lp, t.lo[a]);
        pad_taps(synthesis ? f.syn_hi : f.ana_hi, f.len, Lp, t.hi[a]);
    }
    return t;
}

// Nontemporal output stores: float data whose output rows are whole 128-byte lines (a nontemporal store of a partly covered line
// is a read-modify-write in memory; plain stores of neighbouring tiles merge in L2).  Double never (ndwt_device.h: stream_store).
template <typename T> static int nt_store_ok(long long rs, long long plane, long long bstride, T* const* out, int nout) {
    if (sizeof(T) != 4) return 0;
    const long long line = 128 / (long long)sizeof(T);
    if (rs % line != 0 || plane % line != 0 || bstride % line != 0) return 0;
    for (int b = 0; b < nout; ++b)
        if (((uintptr_t)out[b]) % 128 != 0) return 0;
    return 1;
}

// one fused 3-D launch: what a call site says of it (the rest follows from the plan).  ZMode: the values Fused3Args::z_wrap documents
enum ZMode { kZHalo = 0, kZPeriodic = 1, kZSplitHalo = 2, kZZeroExt = 3 };   // inputs with their z halo | periodic | halo planes in in[1] / in[2] | zero-extended slab
constexpr int kShrinkTLowDetails = 0xFE, kShrinkTHighAll = 0xFF;   // bands shrunk on load (ndwt_denoise): the details of a 3-D level / of the t-low half, every band of the t-high half
// ndwt_denoise's thresholding, done by the synthesis kernels as they load the detail bands: what rec_impl hands down to the launches
// that can (only asked of plans whose every level runs one: fused_shrink_capable).  Every other synthesis passes kNoShrink.
struct ShrinkOnLoad { int mode = 0; double thr = 0; };   // mode: 0 none, 1 soft, 2 hard
constexpr ShrinkOnLoad kNoShrink = {};
static ShrinkOnLoad shrink_on_load(double thr, int mode) { return {mode == NDWT_SHRINK_HARD ? 2 : 1, thr}; }
template <typename T> struct Fused3Launch {
    bool inverse;
    int Lp;
    const T* const* in;                // analysis: in[0] (kZSplitHalo: in[0 .. 2]); synthesis: the 8 bands
    T* const* out;                     // analysis: the 8 bands; synthesis: out[0]
    long long n3;                      // output planes
    long long nbatch = 1, in_bstride = 0, out_bstride = 0;   // volumes of the launch and the scalars between them
    ZMode z = kZPeriodic;
    long long zlo = 0, zhi = 0, zbs = 0;   // kZZeroExt: input planes outside [zlo, zhi) read as zero, batch item i testing plane + i * zbs
    int shrink_mask = 0;               // synthesis: the bands `shrink` applies to
    ShrinkOnLoad shrink = {};
    int dil = 1;                       // tap stride of a dilated level on its sub-lattices
    const double* ttaps = nullptr;     // kRouteFused3FoldT: the t taps of this launch's t-band
};
template <typename T> static int fused3_run(const ndwt_plan* p, const Fused3Launch<T>& l, hipStream_t s) {
    const bool inverse = l.inverse;
    const int Lp = l.Lp, dil = l.dil;
    const T* const* in = l.in;
    T* const* out = l.out;
    const long long in_bstride = l.in_bstride, out_bstride = l.out_bstride;
    Fused3Args<T> a;
    memset(&a, 0, sizeof a);
    if (l.ttaps) {                                        // 4-D analysis, t axis folded in: taps of this launch's t-band, frames = batch items
        for (int j = 0; j < Lp; ++j) a.tt[j] = (T)l.ttaps[j];
    }
    a.zlo = (int)l.zlo;
    a.zhi = (int)(l.z == kZZeroExt ? l.zhi : l.n3 - (Lp - 1));   // (the other modes never read the window)
    a.zbs = (int)l.zbs;
    if (inverse && l.shrink.mode && l.shrink_mask) {      // only reached with a lane-shift synthesis kernel (fused_shrink_capable)
        a.shrink_thr = (T)l.shrink.thr;
        a.shrink_mask = l.shrink_mask;
        a.shrink_hard = l.shrink.mode == 2;
    }
    a.n1 = (int)(p->dims[0] * p->comp);                   // scalars along x (interleaved complex: 2 per element)
    a.n2 = (int)(p->dims[1] / dil);                       // dil > 1: one (y, z) sub-lattice per batch item
    a.n3 = (int)(l.n3 / dil);
    a.nbatch = (int)(dil > 1 ? dil * dil : l.nbatch);
    a.in_bstride = in_bstride;
    a.out_bstride = out_bstride;
    a.z_wrap = l.z;
    a.stamps = p->stamps;
    bool vec4 = (a.n1 % 4 == 0) && (in_bstride % 4 == 0) && (out_bstride % 4 == 0);
    const int nin = inverse ? 8 : (l.z == kZSplitHalo ? 3 : 1), nout = inverse ? 1 : 8;
    for (int b = 0; b < nin; ++b) { a.in[b] = in[b]; vec4 = vec4 && aligned_vec4<T>(in[b]); }
    for (int b = 0; b < nout; ++b) { a.out[b] = out[b]; vec4 = vec4 && aligned_vec4<T>(out[b]); }
#ifdef NDWT_EXP_BANDPAD   // diagnostic build (timing only, results are garbage): skew the band streams against each other
    if (const char* v = getenv("NDWT_EXP_BANDPAD")) {
        const long long pad = atoll(v);
        const int div = getenv("NDWT_EXP_BANDDIV") ? atoi(getenv("NDWT_EXP_BANDDIV")) : 1;   // bands b, b+1, .. b+div-1 keep their distance
        const int mask = getenv("NDWT_EXP_BANDMASK") ? (int)strtol(getenv("NDWT_EXP_BANDMASK"), nullptr, 0) : 0;   // these bands get +pad
        if (inverse && mask) for (int b = 0; b < nin; ++b) a.in[b] = in[b] + ((mask >> b) & 1) * pad;
        else if (inverse) for (int b = 0; b < nin; ++b) a.in[b] = in[b] + (b / div) * pad;
        else for (int b = 0; b < nout; ++b) a.out[b] = out[b] + (b / div) * pad;
    }
#endif
    const Fused3Query q = {sizeof(T) == 8, inverse, vec4, p->uniform_yz, l.ttaps != nullptr, Lp, {p->filt[0].len, p->filt[1].len, p->filt[2].len},
                           dil > 1 ? dil : (int)p->comp, dil, a.n1, a.n2, a.nbatch, p->variant_fwd, p->variant_inv, p->num_cus, p->target_blocks};
    const Fused3Pick k = fused3_select(q);
    if (k.kernel == kNoFused3) return fail(NDWT_ERR_UNSUPPORTED, "internal: no fused 3-D kernel of this variant for tap length %d / this alignment", Lp);
    const int zc_force = p->zchunk_dir[inverse ? 1 : 0] > 0 ? p->zchunk_dir[inverse ? 1 : 0] : p->force_zchunk;
    // more tiles than resident slots: fused3_geometry picks the chunk count with the fewest plane steps over all rounds
    fused3_geometry(a, k.TX, k.TY, Lp, k.target, zc_force);
    if (dil > 1) {
        a.rs = (int)(dil * p->dims[0]);
        a.plane = (long long)dil * p->dims[0] * p->dims[1];
        a.bsplit = dil;
        a.in_bstride = a.out_bstride = p->dims[0];                         // sub-lattice offset along y ...
        a.in_bstride2 = a.out_bstride2 = p->dims[0] * p->dims[1];          // ... and along z
    }
    // (a tile narrower than whole lines -- the 48-wide pair-packed tiles of 20 taps / complex 12 taps -- would put tile edges inside
    // a line: two workgroups' partial nontemporal stores of one line, the read-modify-write case again)
    a.nt = ((long long)k.TX * (long long)sizeof(T)) % 128 == 0 ? nt_store_ok<T>(a.rs, a.plane, out_bstride, out, nout) : 0;
    const void* td = p->taps_dev[inverse ? 1 : 0].ptr;
    if (!td) return fail(NDWT_ERR_UNSUPPORTED, "plan has no device tap table");
    prof_begin(p, inverse ? NDWT_KERNEL_FUSED_SYNTHESIS : NDWT_KERNEL_FUSED_ANALYSIS, s);
    const int rc = launch_fused3_pick(k, a, td, s);   // (-1: no unit has the instance -- after a pick that is an internal error)
    prof_end(p, s, rc);
    if (rc == -1) return fail(NDWT_ERR_UNSUPPORTED, "internal: no fused kernel instantiated for the pick (kernel %d, tap length %d)", (int)k.kernel, Lp);
    if (rc == -2) return fail(NDWT_ERR_UNSUPPORTED, "internal: launch geometry (%d x %d tiles) does not match the kernel's tile shape", k.TX, k.TY);
    if (rc != 0) return fail(NDWT_ERR_HIP, "fused kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return NDWT_OK;
}

// one fused 2-D launch, as a call site describes it
template <typename T> struct Fused2Launch {
    bool inverse;
    int Lp;
    const T* const* in;                // analysis: in[0]; synthesis: the 4 bands
    T* const* out;
    long long n2;                      // output rows
    long long in_bstride = 0, out_bstride = 0;
    bool y_wrap = true;                // false: the inputs carry the y halo (slab mode)
    int dil = 1;                       // tap stride of a dilated level on its row sub-lattices
    long long nbatch = 1;              // images of the launch (a stack: its items, in_bstride / out_bstride apart)
    ShrinkOnLoad shrink = {};          // synthesis: of the 3 detail bands
};
template <typename T> static int fused2_run(const ndwt_plan* p, const Fused2Launch<T>& l, hipStream_t s) {
    const bool inverse = l.inverse;
    const int Lp = l.Lp, dil = l.dil;
    const T* const* in = l.in;
    T* const* out = l.out;
    const long long n2 = l.n2, out_bstride = l.out_bstride;
    Fused2Args<T> a;
    memset(&a, 0, sizeof a);
    a.n1 = (int)(p->dims[0] * p->comp);
    a.n2 = (int)(n2 / dil);                               // dil > 1: the dil row sub-lattices are the batch items
    a.nbatch = dil > 1 ? dil : (int)l.nbatch;
    a.in_bstride = dil > 1 ? p->dims[0] : l.in_bstride;
    a.out_bstride = dil > 1 ? p->dims[0] : out_bstride;
    a.y_wrap = l.y_wrap ? 1 : 0;
    if (inverse && l.shrink.mode) {                      // ndwt_denoise: threshold the 3 detail bands as they are loaded
        a.shrink_thr = (T)l.shrink.thr;
        a.shrink_mask = 0xE;
        a.shrink_hard = l.shrink.mode == 2;
    }
    bool vec4 = (a.n1 % 4 == 0);
    const int nin = inverse ? 4 : 1, nout = inverse ? 1 : 4;
    for (int b = 0; b < nin; ++b) { a.in[b] = in[b]; vec4 = vec4 && aligned_vec4<T>(in[b]); }
    for (int b = 0; b < nout; ++b) { a.out[b] = out[b]; vec4 = vec4 && aligned_vec4<T>(out[b]); }
    const Fused2Query q = {sizeof(T) == 8, inverse, vec4, Lp, dil > 1 ? dil : (int)p->comp, dil, a.n1, (int)n2, p->variant_inv, a.nbatch};
    const Fused2Pick k = fused2_select(q);
    fused2_geometry(a, fused2_tile_width(inverse, Lp, q.ew), Lp, p->target_blocks > 0 ? p->target_blocks * 2 : k.waves, p->force_zchunk);
    if (dil > 1) a.rs = (int)(dil * p->dims[0]);   // 8 waves per CU: one round (measured optimum 1024^2 .. 4096^2)
    a.nt = nt_store_ok<T>(a.rs, a.rs, out_bstride, out, nout);
    const void* td = p->taps_dev[inverse ? 1 : 0].ptr;
    if (!td) return fail(NDWT_ERR_UNSUPPORTED, "plan has no device tap table");
    prof_begin(p, inverse ? NDWT_KERNEL_FUSED_SYNTHESIS : NDWT_KERNEL_FUSED_ANALYSIS, s);
    const int rc = launch_fused2_pick(k, a, td, s);   // (-1, -2: after a pick, internal errors -- see fused3_run)
    prof_end(p, s, rc);
    if (rc == -1) return fail(NDWT_ERR_UNSUPPORTED, "internal: no fused 2-D kernel instantiated for the pick (family %d, tap length %d)", (int)k.family, Lp);
    if (rc == -2) return fail(NDWT_ERR_UNSUPPORTED, "internal: launch geometry does not match the 2-D kernel's tile width %d, or its grid is beyond 2^31 - 1 waves", fused2_tile_width(inverse, Lp, q.ew));
    if (rc != 0) return fail(NDWT_ERR_HIP, "fused 2-D kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return NDWT_OK;
}

// ------------------------------------------------------------------------------------------ levels
// slab mode: the input (every synthesis input) carries the halo planes of the sharded axis p->shard
static SlabMode slab_mode(const ndwt_plan* p, bool slab = true) { return !slab ? kWholeArray : p->shard == p->ndim - 1 ? kSlabOuter : kSlabZ; }
static long long slab_planes(const ndwt_plan* p, long long stride, bool slab) {
    return p->dims[p->shard] + (slab ? (long long)(p->filt[p->shard].len - 1) * stride : 0);
}

// kRouteFused3T, analysis: the t pass over frames of nz_in planes (periodic, or t_wrap = false: the slab's t halo) into two t-bands, the
// second 256 B off a power-of-two distance from the first (see ndwt_band_pitch), then the 3-D level of both halves batched over the frames
template <typename T>
static int analysis_4d(ndwt_plan* p, int Lp, const T* in, T* const* out, long long stride, long long nz_in, ZMode z, bool t_wrap, hipStream_t s) {
    const long long plane = p->comp * p->dims[0] * p->dims[1], band = plane * nz_in * p->dims[3], skew = 256 / (long long)sizeof(T);
    int rc = p->tmp.grow((size_t)(2 * band + skew) * sizeof(T), "for temporaries");
    if (rc) return rc;
    T* lo = (T*)p->tmp.ptr;
    T* hi = lo + band + skew;
    const long long dims_t[NDWT_MAX_DIMS] = {p->dims[0], p->dims[1], nz_in, p->dims[3]};
    rc = axis_pass<T>(p, false, 3, dims_t, stride, t_wrap, in, nullptr, lo, hi, s);
    for (int h = 0; h < 2 && !rc; ++h) {
        const T* ins[8] = {h ? hi : lo};
        Fused3Launch<T> l = {false, Lp, ins, out + 8 * h, p->dims[2]};
        l.nbatch = p->dims[3]; l.in_bstride = plane * nz_in; l.out_bstride = plane * p->dims[2]; l.z = z;
        rc = fused3_run<T>(p, l, s);
    }
    return rc;
}

// kRouteFused3T, synthesis, and the zero-extended forms of the slab entry points: the 3-D level of both t-halves (`frames` frames of nz_in
// coefficient planes -> nz_out planes each) into two t-bands, then the t pass over them -> nt_out frames of nz_out planes.
struct Syn4 {
    long long frames, nz_in, nz_out, nt_out;
    ZMode z = kZPeriodic;
    bool t_wrap = true;
    long long t_pad = 0;               // zero frames on either side of the t-bands (zero-extended t; these bands lie back to back, without the 256 B)
};
template <typename T>
static int synthesis_4d(ndwt_plan* p, int Lp, const T* const* in, T* out, long long stride, const Syn4& f, const ShrinkOnLoad& shrink, hipStream_t s) {
    const long long plane = p->comp * p->dims[0] * p->dims[1], vol3_out = plane * f.nz_out, pad = f.t_pad * vol3_out;
    const long long band = (f.frames + 2 * f.t_pad) * vol3_out, skew = f.t_pad ? 0 : 256 / (long long)sizeof(T);
    int rc = p->tmp.grow((size_t)(2 * band + skew) * sizeof(T), "for temporaries");
    if (rc) return rc;
    T* bands[2] = {(T*)p->tmp.ptr, (T*)p->tmp.ptr + band + skew};
    for (int h = 0; h < 2 && pad; ++h) {
        HIP_TRY(hipMemsetAsync(bands[h], 0, (size_t)pad * sizeof(T), s));
        HIP_TRY(hipMemsetAsync(bands[h] + band - pad, 0, (size_t)pad * sizeof(T), s));
    }
    for (int h = 0; h < 2; ++h) {                          // in[0] = approximation: the t-low half shrinks its details, the t-high half every band
        T* outs[8] = {bands[h] + pad};
        Fused3Launch<T> l = {true, Lp, in + 8 * h, outs, f.nz_out};
        l.nbatch = f.frames; l.in_bstride = plane * f.nz_in; l.out_bstride = vol3_out; l.z = f.z; l.zhi = f.nz_in;
        l.shrink_mask = h ? kShrinkTHighAll : kShrinkTLowDetails; l.shrink = shrink;
        rc = fused3_run<T>(p, l, s);
        if (rc) return rc;
    }
    const long long dims_t[NDWT_MAX_DIMS] = {p->dims[0], p->dims[1], f.nz_out, f.nt_out};
    return axis_pass<T>(p, true, 3, dims_t, stride, f.t_wrap, bands[0], bands[1], out, nullptr, s);
}

// analysis of one level: in (vol scalars, + halo planes in slab mode) -> 2^d bands
template <typename T>
static int analysis_level(ndwt_plan* p, const T* in, T* const* out, long long stride, bool slab, hipStream_t s) {
    // (a stack is never a slab: vol_in and vol_out are then the scalars of ONE item, the launch's batch stride both ways)
    const long long n_sh = slab_planes(p, stride, slab), vol_out = p->item_vol(), vol_in = vol_out / p->dims[p->shard] * n_sh;
    const bool on_z = p->shard == 2;                       // (of a 4-D level: the sharded axis is z, else t)
    const T* ins[8] = {in};
    LevelRoute r = level_route(sel(p), stride, 0, slab_mode(p, slab));
    if (r.kind == kRouteFused3FoldT) {
        bool ok = aligned_vec4<T>(in);
        for (int b = 0; ok && b < 16; ++b) ok = aligned_vec4<T>(out[b]);
        if (!ok) r.kind = kRouteFused3T;
    }
    switch (r.kind) {
        case kRouteFused3Dilated: {
            Fused3Launch<T> l = {false, r.Lp, ins, out, p->dims[2]};
            l.dil = (int)stride;
            return fused3_run<T>(p, l, s);
        }
        case kRouteFused3: {
            Fused3Launch<T> l = {false, r.Lp, ins, out, p->dims[2]};
            l.nbatch = p->items(); l.in_bstride = vol_in; l.out_bstride = vol_out; l.z = slab ? kZHalo : kZPeriodic;
            return fused3_run<T>(p, l, s);
        }
        // A/B variant 7 (Plan.set_variant(fwd=7)) -- MEASURED AND NOT THE DEFAULT: the t axis folded into the fused launches, each raw plane a
        // workgroup takes being the t-filtered combination of the same plane of L frames (read where the neighbouring frames' workgroups
        // read them: L2), one launch per t-band: 17 volume transfers per level instead of 21 (nd_dwt_4D.m:394-467).  The bytes go down,
        // the time goes up: cfg5 (256^3 x 32, db4) 6.55 ms per launch against 3.41 ms + half of the 1.36 ms t pass -- the 8 loads per lane
        // and plane (against 1) go through the same per-CU vector-memory pipe as the 4 stores, and that pipe is what bounds the kernel
        // (68.6 ms per dec+rec step against 53.5 ms).
        case kRouteFused3FoldT: {
            const long long vol3 = p->vol / p->dims[3];
            double tt[2][kMaxTaps];
            pad_taps(p->filt[3].ana_lo, p->filt[3].len, r.Lp, tt[0]);
            pad_taps(p->filt[3].ana_hi, p->filt[3].len, r.Lp, tt[1]);
            for (int h = 0; h < 2; ++h) {
                Fused3Launch<T> l = {false, r.Lp, ins, out + 8 * h, p->dims[2]};
                l.nbatch = p->dims[3]; l.in_bstride = l.out_bstride = vol3; l.ttaps = tt[h];
                const int rc = fused3_run<T>(p, l, s);
                if (rc) return rc;
            }
            return NDWT_OK;
        }
        case kRouteFused3T: return analysis_4d<T>(p, r.Lp, in, out, stride, on_z ? n_sh : p->dims[2], slab && on_z ? kZHalo : kZPeriodic, !slab || on_z, s);
        case kRouteFused2Dilated: {
            Fused2Launch<T> l = {false, r.Lp, ins, out, p->dims[1]};
            l.dil = (int)stride;
            return fused2_run<T>(p, l, s);
        }
        case kRouteFused2: {
            Fused2Launch<T> l = {false, r.Lp, ins, out, p->dims[1]};
            l.nbatch = p->items(); l.in_bstride = vol_in; l.out_bstride = vol_out; l.y_wrap = !slab;
            return fused2_run<T>(p, l, s);
        }
        default: return per_axis_level<T>(p, false, ins, out, stride, slab, s);   // kRoutePerAxis
    }
}

template <typename T>
static int synthesis_level(ndwt_plan* p, const T* const* in, T* out, long long stride, bool slab, const ShrinkOnLoad& shrink, hipStream_t s) {
    const long long n_sh = slab_planes(p, stride, slab), vol_out = p->item_vol(), vol_in = vol_out / p->dims[p->shard] * n_sh;
    const bool on_z = p->shard == 2;
    T* outs[8] = {out};
    const LevelRoute r = level_route(sel(p), stride, 1, slab_mode(p, slab));
    switch (r.kind) {
        case kRouteFused3Dilated: {
            Fused3Launch<T> l = {true, r.Lp, in, outs, p->dims[2]};
            l.dil = (int)stride;
            return fused3_run<T>(p, l, s);
        }
        case kRouteFused3: {
            Fused3Launch<T> l = {true, r.Lp, in, outs, p->dims[2]};
            l.nbatch = p->items(); l.in_bstride = vol_in; l.out_bstride = vol_out; l.z = slab ? kZHalo : kZPeriodic; l.shrink_mask = kShrinkTLowDetails; l.shrink = shrink;
            return fused3_run<T>(p, l, s);
        }
        case kRouteFused3T: {                              // (a slab on t: the 3-D part runs on the halo frames too)
            Syn4 f = {on_z ? p->dims[3] : n_sh, on_z ? n_sh : p->dims[2], p->dims[2], p->dims[3]};
            f.z = slab && on_z ? kZHalo : kZPeriodic; f.t_wrap = !slab || on_z;
            return synthesis_4d<T>(p, r.Lp, in, out, stride, f, shrink, s);
        }
        case kRouteFused2Dilated: {
            Fused2Launch<T> l = {true, r.Lp, in, outs, p->dims[1]};
            l.dil = (int)stride;
            return fused2_run<T>(p, l, s);
        }
        case kRouteFused2: {
            Fused2Launch<T> l = {true, r.Lp, in, outs, p->dims[1]};
            l.nbatch = p->items(); l.in_bstride = vol_in; l.out_bstride = vol_out; l.y_wrap = !slab; l.shrink = shrink;
            return fused2_run<T>(p, l, s);
        }
        default: return per_axis_level<T>(p, true, in, outs, stride, slab, s);   // kRoutePerAxis
    }
}

// --------------------------------------------------------------------------------- multi-level
// band bookkeeping of nddwt.c:210,225-234 / nd_dwt_3D.m:178-186: level `lev` (1 = finest) stores its
// 2^d-1 detail bands at [1 + (2^d-1)(level-lev), ...); the coarsest approximation is band 0.  Unlike
// the reference there is no cat() copy (nd_dwt_3D.m:184) and no in-place overwrite of the input.
// bs: distance between consecutive bands of y in scalars (p->vol = the packed reference layout; larger = pitched)
// ---- two or three levels of an image in one launch (Fwd2C / Inv2C, ndwt_device.h; when: cascade2_levels).  Shared by both directions:
// the tiling (one round of `per_cu` waves per CU -- analysis 8, synthesis 4: DESIGN.md 4 -- in equal chunks of at least nlev (Lp - 1) rows:
// the march-in is at most half of a wave's steps; force_zchunk = rows per wave), profiling, the launch and its error mapping.
// A stack: the items share the round -- chunks per item = waves / (ntx * items), at least 1 -- and the grid is ntx * nyc * items waves.
// Returns 0, or -1: no instance, or a stack whose grid the launch cannot express (the caller takes one launch per level)
template <class Args, class Launch> static int cascade2_launch(ndwt_plan* p, Args& a, bool inverse, int WX, int min_chunk, int per_cu, hipStream_t s, Launch&& launch) {
    a.ntx = (a.n1 + WX - 1) / WX;
    const int waves = p->target_blocks > 0 ? p->target_blocks : p->num_cus * per_cu;
    const long long items = p->items(), per_chunk = a.ntx * items;
    const int chunks = waves / per_chunk > 1 ? (int)(waves / per_chunk) : 1;
    int yc = (a.n2 + chunks - 1) / chunks;
    if (yc < min_chunk) yc = min_chunk;
    if (p->force_zchunk > 0) yc = p->force_zchunk;
    if (yc > a.n2) yc = a.n2;
    a.nyc = (a.n2 + yc - 1) / yc;
    a.ychunk = (a.n2 + a.nyc - 1) / a.nyc;
    a.nyc = (a.n2 + a.ychunk - 1) / a.ychunk;
    a.nbatch = (int)items;
    a.bstride = p->item_vol();
    if ((long long)a.ntx * a.nyc * items > 0x7fffffffLL) return -1;
    const void* td = p->taps_dev[inverse ? 1 : 0].ptr;
    if (!td) return fail(NDWT_ERR_UNSUPPORTED, "plan has no device tap table");
    prof_begin(p, inverse ? NDWT_KERNEL_FUSED_SYNTHESIS : NDWT_KERNEL_FUSED_ANALYSIS, s);
    const int rc = launch(td);
    prof_end(p, s, rc);
    if (rc == -2) return fail(NDWT_ERR_UNSUPPORTED, "internal: launch geometry does not match the cascaded 2-D kernel's tile");
    if (rc > 0) return fail(NDWT_ERR_HIP, "cascaded 2-D %s launch failed: %s", inverse ? "synthesis" : "analysis", hipGetErrorString((hipError_t)rc));
    return rc;
}
// (interleaved complex: rows of dims[0] * comp scalars, the x taps step over the pairs -- the kernels' EW)
template <typename T> static int cascade2_run(ndwt_plan* p, int Lp, int nlev, const T* in, T* const* out, hipStream_t s) {
    Fused2CArgs<T> a;
    memset(&a, 0, sizeof a);
    a.in = in;
    a.n1 = a.rs = (int)(p->dims[0] * p->comp);
    a.n2 = (int)p->dims[1];
    bool aligned = aligned_vec4<T>(in);
    for (int b = 0; b < 1 + 3 * nlev; ++b) { a.out[b] = out[b]; aligned = aligned && aligned_vec4<T>(out[b]); }
    if (!aligned) return -1;                              // not this data: one launch per level
    a.nt = nt_store_ok<T>(a.rs, a.rs, 0, out, 1 + 3 * nlev);   // (the item stride is rows of rs scalars: whole lines wherever rs is)
    a.mode = p->variant_fwd == kFwdCascadeMode1 ? 1 : 0;
    const Cascade2Instance k = {false, sizeof(T) == 8, (int)p->comp, Lp, nlev, 0};
    return cascade2_launch(p, a, false, cascade2_tile_width(k), nlev * (Lp - 1), 8, s, [&](const void* td) { return launch_cascade2(k, a, td, s); });
}

// ---- what the launches of the two 1-D cascades share (Fwd1C / Inv1C and FwdMC / InvMC; the caller has laid out the geometry in `a`): the
// band pointers into a.in / a.out -- analysis in[0] and out[0 .. nlev], synthesis in[0 .. nlev] and out[0], as Fused1CArgs and MarchCArgs
// document them -- and their alignment, the device tap table `td` where the family reads one (needs_taps),
// profiling, the launch and its error mapping.  Returns 0, or -1: not this data (a pointer off the 16- / 32-byte groups) or no instance
// -- the caller takes one launch per level
template <typename T, class Args, class Launch>
static int cascade1d_launch(const ndwt_plan* p, Args& a, bool inverse, int nlev, const T* const* in, T* const* out, const char* what,
                            bool needs_taps, const void* td, hipStream_t s, Launch&& launch) {
    bool aligned = true;
    for (int b = 0; b < (inverse ? 1 + nlev : 1); ++b) { a.in[b] = in[b]; aligned = aligned && aligned_vec4<T>(in[b]); }
    for (int b = 0; b < (inverse ? 1 : 1 + nlev); ++b) { a.out[b] = out[b]; aligned = aligned && aligned_vec4<T>(out[b]); }
    if (!aligned) return -1;
    if (needs_taps && !td) return fail(NDWT_ERR_UNSUPPORTED, "plan has no device tap table");
    prof_begin(p, inverse ? NDWT_KERNEL_FUSED_SYNTHESIS : NDWT_KERNEL_FUSED_ANALYSIS, s);
    const int rc = launch();
    prof_end(p, s, rc);
    if (rc > 0) return fail(NDWT_ERR_HIP, "cascaded %s %s launch failed: %s", what, inverse ? "synthesis" : "analysis", hipGetErrorString((hipError_t)rc));
    return rc < 0 ? -1 : 0;
}

// ---- two to four levels of the signals of a batched 1-D plan in one launch (Fwd1C / Inv1C, ndwt_device_1d.h; when: cascade1_levels).
// in / out as Fused1CArgs documents them.  Returns 0, or -1 as cascade1d_launch does (no instance: also a launch the kernel's tiling
// cannot express)
template <typename T> static int cascade1_run(ndwt_plan* p, bool inverse, int L, int nlev, const T* const* in, T* const* out, hipStream_t s) {
    Fused1CArgs<T> a;
    memset(&a, 0, sizeof a);
    const Cascade1Instance k = {inverse, sizeof(T) == 8, (int)p->comp, L, nlev};
    const int WX = cascade1_tile_width(k);
    a.row = p->dims[0] * p->comp;
    a.outer = p->howmany;
    a.nseg = (a.row + WX - 1) / WX;
    const void* const td = p->taps_dev[inverse ? 1 : 0].ptr;
    return cascade1d_launch(p, a, inverse, nlev, in, out, "1-D", true, td, s, [&] { return launch_cascade1(k, a, td, s); });
}

// ---- dec, per-band thresholding and rec of the signals of a batched 1-D plan in one launch (Den1C, ndwt_device_1d.h; when:
// denoise1_levels).  thr: one threshold per band of the coefficient array (band 0 the approximation, then the detail bands coarsest
// level first), converted as shrink_run converts them.  Returns 0, or -1: not this data -- x or out off the 16- / 32-byte groups, x and
// out overlapping (a wave reads halo scalars that another wave's store may already have replaced), no instance, no tap table, or a grid
// beyond 2^31 - 1 workgroups -- and the caller takes the general route
// thr_rows: null, or the device table [signals][5] of ndwt_denoise_bands_items, every row in the order of a.thr -- Den1C<.., ROWTHR>
template <typename T> static int denoise1_run(ndwt_plan* p, int L, int nlev, const T* x, T* out, const double* thr, int mode, hipStream_t s,
                                              const T* thr_rows = nullptr) {
    const char *xb = (const char*)x, *ob = (const char*)out;
    const size_t nbytes = (size_t)p->vol * sizeof(T);
    if (!aligned_vec4<T>(x) || !aligned_vec4<T>(out) || !(xb + nbytes <= ob || ob + nbytes <= xb)) return -1;
    const void* td = p->taps_den1.ptr;
    if (!td) return -1;
    Den1CArgs<T> a;
    memset(&a, 0, sizeof a);
    a.in[0] = x;
    a.out[0] = out;
    if (thr) {
        a.thr[0] = (T)thr[0];
        for (int l = 0; l < nlev; ++l) a.thr[1 + l] = (T)thr[1 + (nlev - 1 - l)];   // cascade level l (0 = finest) is transform level l + 1: band 1 + (nlev - (l + 1))
    }
    a.thr_rows = thr_rows;
    a.hard = mode == NDWT_SHRINK_HARD;
    const Den1Instance k = {sizeof(T) == 8, (int)p->comp, L, nlev};
    const int WX = den1_tile_width(k);
    a.row = p->dims[0] * p->comp;
    a.outer = p->howmany;
    a.nseg = (a.row + WX - 1) / WX;
    if ((a.outer * a.nseg + 3) / 4 > 0x7fffffffLL) return -1;
    prof_begin(p, NDWT_KERNEL_FUSED_SYNTHESIS, s);
    const int rc = thr_rows ? launch_den1r(k, a, td, s) : launch_den1(k, a, td, s);
    prof_end(p, s, rc);
    if (rc > 0) return fail(NDWT_ERR_HIP, "one-launch denoise failed: %s", hipGetErrorString((hipError_t)rc));
    return rc < 0 ? -1 : 0;
}

// ---- two to four levels of the one strided axis of a plan over interleaved samples in one march (FwdMC / InvMC, ndwt_device_axis.h;
// when: cascadem_levels).  in / out as MarchCArgs documents them.  The chunking is march_chunks (ndwt_select.h) with a floor of
// 4 nlev (L - 1) planes -- the march-in is at most a quarter of a thread's planes; force_zchunk / zchunk_dir = planes per chunk.  Returns 0, or -1 as cascade1d_launch does, or for a grid beyond 2^31 - 1
// workgroups
template <typename T> static int cascadem_run(ndwt_plan* p, bool inverse, int L, int nlev, const T* const* in, T* const* out, hipStream_t s) {
    MarchCArgs<T> a;
    memset(&a, 0, sizeof a);
    a.inner = p->comp * p->inner;
    if (a.inner % 4 != 0) return -1;
    a.n = p->dims[0];
    a.outer = p->items();
    a.ngroups = a.inner / 4;
    const long long iblocks = (a.ngroups * a.outer + 255) / 256;
    const MarchChunks c = march_chunks(a.n, iblocks, 4LL * nlev * (L - 1), p->zchunk_dir[inverse ? 1 : 0] > 0 ? p->zchunk_dir[inverse ? 1 : 0] : p->force_zchunk);
    a.chunk = c.chunk;
    a.nchunks = c.nchunks;
    if (iblocks * a.nchunks > 0x7fffffffLL) return -1;
    const AxisFilter& f = p->filt[0];
    const CascadeMInstance k = {inverse, sizeof(T) == 8, L, nlev};
    return cascade1d_launch(p, a, inverse, nlev, in, out, "march", false, nullptr, s,
                            [&] { return launch_cascadem(k, a, inverse ? f.syn_lo : f.ana_lo, inverse ? f.syn_hi : f.ana_hi, s); });
}

// detail band b (1 .. 2^d - 1) of level `lev` in the coefficients y of a `level`-level transform (the bookkeeping above)
template <typename T> static T* detail_band(const ndwt_plan* p, T* y, long long bs, int level, int lev, int b) {
    return y + (long long)(1 + ((1 << p->ndim) - 1) * (level - lev) + (b - 1)) * bs;
}

// the detail bands of `n` levels behind slot 0 of `bands`, the 2^d - 1 of a level together: level `first`, then first + step, .. -- the
// order the launch's Args document: coarsest level first (Fused2CArgs, Fused2CIArgs, the synthesis of Fused1CArgs and MarchCArgs)
// everywhere but in the analysis of the two 1-D cascades
template <typename B> static void level_bands(const ndwt_plan* p, B* y, long long bs, int level, int first, int step, int n, B** bands) {
    const int nd = (1 << p->ndim) - 1;
    for (int c = 0; c < n; ++c)
        for (int b = 1; b <= nd; ++b) bands[1 + nd * c + (b - 1)] = detail_band(p, y, bs, level, first + step * c, b);
}

// The walk over the levels, finest first: cascade_route names the next launch -- levels lev .. last in one, or level lev alone by
// level_route.  "None" is final within a call: a cascade that does not take `left` levels takes no fewer either (tests/
// test_dispatch_select.py checks that of cascade_route), so the walk stops asking, as it does after a cascade that declined its data.
// The approximations between launches alternate between the plan's two scratch volumes (a launch never writes the one it reads); the
// last launch writes band 0 of y.
template <typename T> static int dec_impl(ndwt_plan* p, const T* x, T* y, long long bs, int level, hipStream_t s) {
    const SelPlan sp = sel(p);
    const T* cur = x;
    int lev = 1, pp = 0;                                  // pp: the scratch volume the next launch writes
    bool cascades = true;                                 // until none claims the levels left, or one declines
    while (lev <= level) {
        const CascadeRoute r = cascades ? cascade_route(sp, false, level - lev + 1) : CascadeRoute{kCascadeNone, 0, 0};
        if (r.kind == kCascadeNone) cascades = false;
        const int n = r.kind == kCascadeNone ? 1 : r.nlev, last = lev + n - 1;
        const T* in[1] = {cur};
        T* out[16];
        out[0] = (last == level) ? y : (T*)p->approx(pp);
        if (r.kind == kCascadeImage2) level_bands(p, y, bs, level, last, -1, n, out);
        else level_bands(p, y, bs, level, lev, +1, n, out);
        int rc;
        switch (r.kind) {
            case kCascadeRows1: rc = cascade1_run<T>(p, false, r.L, n, in, out, s); break;
            case kCascadeMarch: rc = cascadem_run<T>(p, false, r.L, n, in, out, s); break;
            case kCascadeImage2: rc = cascade2_run<T>(p, r.L, n, cur, out, s); break;
            default: rc = analysis_level<T>(p, cur, out, level_stride(p, lev), false, s);
        }
        if (rc == -1 && r.kind != kCascadeNone) { cascades = false; continue; }   // not this data: one launch per level from here on
        if (rc) return rc;
        cur = out[0];
        pp ^= 1;
        lev = last + 1;
    }
    return NDWT_OK;
}

// the synthesis side of the cascade (Inv2C): in[0] = approximation of the coarsest level, then the detail bands coarsest level first
template <typename T> static int cascade2_rec_run(ndwt_plan* p, int Lp, int nlev, const T* const* in, T* out, const ShrinkOnLoad& shrink, hipStream_t s) {
    Fused2CIArgs<T> a;
    memset(&a, 0, sizeof a);
    a.out = out;
    a.n1 = a.rs = (int)(p->dims[0] * p->comp);
    a.n2 = (int)p->dims[1];
    bool aligned = aligned_vec4<T>(out);
    for (int b = 0; b < 1 + 3 * nlev; ++b) { a.in[b] = in[b]; aligned = aligned && aligned_vec4<T>(in[b]); }
    if (!aligned) return -1;
    T* outs[1] = {out};
    a.nt = nt_store_ok<T>(a.rs, a.rs, 0, outs, 1);
    if (shrink.mode) {                                    // ndwt_denoise: threshold the detail bands as their rows are loaded
        a.shrink_on = 1;
        a.shrink_thr = (T)shrink.thr;
        a.shrink_hard = shrink.mode == 2;
    }
    const Cascade2Instance k = {true, sizeof(T) == 8, (int)p->comp, Lp, nlev, cascade2_rec_depth(sel(p), Lp, nlev)};
    return cascade2_launch(p, a, true, cascade2_tile_width(k), nlev * (Lp - 1), 4, s, [&](const void* td) { return launch_cascade2(k, a, td, s); });
}

// The walk back, coarsest level first: levels lev .. low in one launch, or level lev alone; the last launch writes x.  shrink: see
// ShrinkOnLoad.
template <typename T> static int rec_impl(ndwt_plan* p, const T* y, long long bs, T* x, int level, const ShrinkOnLoad& shrink, hipStream_t s) {
    const SelPlan sp = sel(p);
    const T* prev = y;                                    // band 0
    int lev = level, pp = 0;                              // coarsest level still to be synthesised; pp: the scratch volume the next launch writes
    bool cascades = true;                                 // until none claims the levels left, or one declines
    while (lev >= 1) {
        const CascadeRoute r = cascades ? cascade_route(sp, true, lev) : CascadeRoute{kCascadeNone, 0, 0};
        if (r.kind == kCascadeNone) cascades = false;
        const int n = r.kind == kCascadeNone ? 1 : r.nlev, low = lev - n + 1;
        const T* in[16];
        in[0] = prev;
        level_bands(p, y, bs, level, lev, -1, n, in);
        T* dst[1] = {(low == 1) ? x : (T*)p->approx(pp)};
        int rc;
        switch (r.kind) {
            case kCascadeRows1: rc = cascade1_run<T>(p, true, r.L, n, in, dst, s); break;
            case kCascadeMarch: rc = cascadem_run<T>(p, true, r.L, n, in, dst, s); break;
            case kCascadeImage2: rc = cascade2_rec_run<T>(p, r.L, n, in, dst[0], shrink, s); break;
            default: rc = synthesis_level<T>(p, in, dst[0], level_stride(p, lev), false, shrink, s);
        }
        if (rc == -1 && r.kind != kCascadeNone) { cascades = false; continue; }   // not this data: one launch per level from here on
        if (rc) return rc;
        prev = dst[0];
        pp ^= 1;
        lev = low - 1;
    }
    return NDWT_OK;
}

// What sizes a host buffer, a handle or a slab by the dimensions of ONE array does not know the signals of a batched plan
// (ndwt_plan_create_many): those entry points refuse it (include/ndwt.h lists them)
static int refuse_batched(const ndwt_plan* p, const char* what) {
    if (p && p->howmany > 0)
        return fail(NDWT_ERR_UNSUPPORTED, "%s is not available on a batched plan (ndwt_plan_create_many): use the device-pointer entry points", what);   // (a stack too)
    return NDWT_OK;
}

static int check_level(const ndwt_plan* p, int level) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    if (level < 1 || level > p->max_level)
        return fail(NDWT_ERR_INVALID_ARG, "level %d outside 1..max_level=%d of this plan", level, p->max_level);
    if (p->thin_slab)
        return fail(NDWT_ERR_FILTER_TOO_LONG, "this slab plan is thinner than its outer-axis filter: only the *_slab entry points apply");
    return NDWT_OK;
}

// fused 3-D slab forms that avoid haloed copies (multi-GPU fast path)
static int slab_fast_ok(const ndwt_plan* p, int stride, int* Lp) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    if (const int rc = refuse_batched(p, "a slab entry point")) return rc;
    if (p->ndim != 3 || !(*Lp = slab_fused3(sel(p), stride, -1, kSlabOuter)))
        return fail(NDWT_ERR_UNSUPPORTED, "split/extended slab entry points need a fused 3-D plan whose outer-axis filter is the longest");
    return NDWT_OK;
}

template <typename T> static int slab_ext_impl(ndwt_plan* p, int Lp, const void* const* in, void* out, hipStream_t s) {
    T* outs[8] = {(T*)out};
    const long long n_out = p->dims[2] + (Lp - 1);
    Fused3Launch<T> l = {true, Lp, (const T* const*)in, outs, n_out};
    l.in_bstride = p->vol; l.out_bstride = p->vol / p->dims[2] * n_out; l.z = kZZeroExt; l.zhi = p->dims[2];
    return fused3_run<T>(p, l, s);
}


// --------------------------------------------------------------------------- shrinkage of detail bands
// Element-wise, in place, 1 read + 1 write per coefficient (HBM-bound); the arithmetic is shrink_group (ndwt_shrink.h).
// VEC: 4 scalars per thread and step (16-byte / 32-byte accesses; pointer aligned, n a multiple of 4); else one group
template <typename T, int COMP, bool VEC>
__global__ void __launch_bounds__(256) shrink_kernel(T* __restrict__ y, long long n_scalars, T thr, int hard) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (VEC) {
        typedef typename VecT<T>::v4 v4;
        v4* yv = reinterpret_cast<v4*>(y);
        for (long long i = t0; i < n_scalars / 4; i += stride) {
            v4 c = yv[i];
            T e[4] = {c[0], c[1], c[2], c[3]};
#pragma unroll
            for (int k = 0; k < 4; k += COMP) shrink_group<T, COMP>(e + k, thr, hard);
            yv[i] = v4{e[0], e[1], e[2], e[3]};
        }
    } else {
        for (long long i = t0; i < n_scalars / COMP; i += stride) shrink_group<T, COMP>(y + i * COMP, thr, hard);
    }
}

template <typename T> static int shrink_run(ndwt_plan* p, T* d, long long n, double thr, int mode, hipStream_t s);
template <typename T> static int shrink_impl(ndwt_plan* p, T* y, long long bs, int level, double thr, int mode, hipStream_t s) {
    const long long nb = ndwt_num_bands(p->ndim, level);
    // band 0 (coarsest approximation) is left as it is; packed bands are one run, pitched ones a launch per band
    if (bs == p->vol) return shrink_run<T>(p, y + p->vol, (nb - 1) * p->vol, thr, mode, s);
    for (long long b = 1; b < nb; ++b) {
        int rc = shrink_run<T>(p, y + b * bs, p->vol, thr, mode, s);
        if (rc) return rc;
    }
    return NDWT_OK;
}
template <typename T> static int shrink_run(ndwt_plan* p, T* d, long long n, double thr, int mode, hipStream_t s) {
    const bool vec = aligned_vec4<T>(d) && n % 4 == 0;
    long long blocks = ((vec ? n / 4 : n / p->comp) + 255) / 256;
    const long long cap = (long long)p->num_cus * 16;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    const dim3 g((unsigned)blocks), b(256);
    trace_plain(g, b, "shrink_kernel", trace_scalar<T>(), (int)p->comp, vec);
    if (p->comp == 2) {
        if (vec) hipLaunchKernelGGL((shrink_kernel<T, 2, true>), g, b, 0, s, d, n, (T)thr, mode);
        else hipLaunchKernelGGL((shrink_kernel<T, 2, false>), g, b, 0, s, d, n, (T)thr, mode);
    } else {
        if (vec) hipLaunchKernelGGL((shrink_kernel<T, 1, true>), g, b, 0, s, d, n, (T)thr, mode);
        else hipLaunchKernelGGL((shrink_kernel<T, 1, false>), g, b, 0, s, d, n, (T)thr, mode);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(NDWT_ERR_HIP, "shrink kernel launch failed: %s", hipGetErrorString(e));
    return NDWT_OK;
}

// 4-D slab, zero-extended synthesis (scatter scheme of the t-sharded driver): the 3-D part is local to every frame, so
// the 16 bands of the slab are synthesised to the two t-bands (a, d) for the local frames only, in buffers that carry
// L-1 zero frames on each side; the t-axis pass over them (slab mode: it reads L-1 frames more than it writes) yields the
// n_local + L-1 frames of the zero-extended result.
template <typename T> static int slab_ext4_impl(ndwt_plan* p, int Lp, const void* const* in, void* out, hipStream_t s) {
    const long long n = p->dims[3], h = p->filt[3].len - 1;
    Syn4 f = {n, p->dims[2], p->dims[2], n + h};
    f.t_wrap = false; f.t_pad = h;
    return synthesis_4d<T>(p, Lp, (const T* const*)in, (T*)out, 1, f, kNoShrink, s);
}

// a run of output planes of the slab transform (the caller offsets the pointers): what lets the halo exchange
// overlap with the planes that do not depend on it
template <typename T>
static int slab_analysis_part_impl(ndwt_plan* p, int Lp, const void* in, const void* hb, const void* ha, void* const* out,
                                   long long n_planes, hipStream_t s) {
    const T* ins[8] = {(const T*)in, (const T*)hb, (const T*)ha};
    Fused3Launch<T> l = {false, Lp, ins, (T* const*)out, n_planes};
    l.in_bstride = l.out_bstride = p->vol; l.z = kZSplitHalo;
    return fused3_run<T>(p, l, s);
}

template <typename T>
static int slab_analysis_runs_impl(ndwt_plan* p, int Lp, const void* in, void* const* out, long long n_planes, long long n_runs,
                                   long long run_stride, hipStream_t s) {
    const long long plane = p->vol / p->dims[2];
    const T* ins[8] = {(const T*)in};
    Fused3Launch<T> l = {false, Lp, ins, (T* const*)out, n_planes};
    l.nbatch = n_runs; l.in_bstride = l.out_bstride = run_stride * plane; l.z = kZHalo;
    return fused3_run<T>(p, l, s);
}

// run r: planes [e0 + r*e_stride, +n_out) of the zero-extended synthesis of n_in coefficient planes -> out + r*n_out planes
template <typename T>
static int slab_synthesis_runs_impl(ndwt_plan* p, int Lp, const void* const* in, long long n_in, long long e0, long long e_stride,
                                    long long n_runs, long long n_out, void* out, hipStream_t s) {
    const long long plane = p->vol / p->dims[2];
    const T* ins[8];
    for (int b = 0; b < 8; ++b) ins[b] = (const T*)in[b] + e0 * plane;      // never dereferenced outside [0, n_in)
    T* outs[8] = {(T*)out};
    Fused3Launch<T> l = {true, Lp, ins, outs, n_out};
    l.nbatch = n_runs; l.in_bstride = e_stride * plane; l.out_bstride = n_out * plane;
    l.z = kZZeroExt; l.zlo = -e0; l.zhi = n_in - e0; l.zbs = e_stride;
    return fused3_run<T>(p, l, s);
}

// ------------------------------------------------------------------------------------------ C ABI
// ---- several runs of planes copied / added in one launch (include/ndwt.h: ndwt_slab_segments) ----
namespace {
struct SegArgs {
    void* dst[NDWT_MAX_SEGMENTS];
    const void* src[NDWT_MAX_SEGMENTS];
    long long count[NDWT_MAX_SEGMENTS];      // in units of V
};
// blockIdx.y = run; 16-byte accesses (V = 4 floats / 2 doubles) where every run allows them, scalars otherwise
template <typename V, bool ADD>
__global__ __launch_bounds__(256) void segments_kernel(const SegArgs a) {
    V* __restrict__ d = (V*)a.dst[blockIdx.y];
    const V* __restrict__ s = (const V*)a.src[blockIdx.y];
    const long long n = a.count[blockIdx.y], step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        if constexpr (ADD) d[i] = d[i] + s[i];
        else d[i] = s[i];
    }
}
// ---- the strided form (include/ndwt.h: ndwt_slab_segments_strided): nrep repetitions of every run, repetition q at q * stride in
// both buffers -- the planes of a z-slab are one run per frame.  blockIdx.y = run, blockIdx.z = repetition; 16-byte accesses over
// the whole 16-byte groups of a run whose two sides are 16-byte aligned in every repetition, scalars for the tail and elsewhere.
struct SegStridedArgs {
    void* dst[NDWT_MAX_SEGMENTS];
    const void* src[NDWT_MAX_SEGMENTS];
    long long count[NDWT_MAX_SEGMENTS];      // scalars
    long long dst_stride[NDWT_MAX_SEGMENTS], src_stride[NDWT_MAX_SEGMENTS];
    int vec[NDWT_MAX_SEGMENTS];
    long long nrep;
};
template <typename T, typename V, bool ADD>
__global__ __launch_bounds__(256) void segments_strided_kernel(const SegStridedArgs a) {
    constexpr int PER = (int)(sizeof(V) / sizeof(T));
    const int r = blockIdx.y;
    const long long n = a.count[r];
    const long long nv = a.vec[r] ? n / PER : 0;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
    for (long long q = blockIdx.z; q < a.nrep; q += gridDim.z) {
        T* __restrict__ d = (T*)a.dst[r] + q * a.dst_stride[r];
        const T* __restrict__ s = (const T*)a.src[r] + q * a.src_stride[r];
        for (long long i = t0; i < nv; i += step) {
            if constexpr (ADD) ((V*)d)[i] = ((V*)d)[i] + ((const V*)s)[i];
            else ((V*)d)[i] = ((const V*)s)[i];
        }
        for (long long i = nv * PER + t0; i < n; i += step) {
            if constexpr (ADD) d[i] = d[i] + s[i];
            else d[i] = s[i];
        }
    }
}
template <typename T> int segments_strided_launch(int op, int nseg, void* const* dst, const void* const* src, const int64_t* count,
                                                  long long nrep, const int64_t* dst_stride, const int64_t* src_stride, hipStream_t st) {
    typedef typename std::conditional<sizeof(T) == 4, typename VecT<T>::v4, typename VecT<T>::v2>::type V;
    constexpr int per = 16 / (int)sizeof(T);
    SegStridedArgs a;
    memset(&a, 0, sizeof a);
    long long most = 1;
    for (int i = 0; i < nseg; ++i) {
        a.dst[i] = dst[i];
        a.src[i] = src[i];
        a.count[i] = count[i];
        a.dst_stride[i] = dst_stride[i];
        a.src_stride[i] = src_stride[i];
        a.vec[i] = (uintptr_t)dst[i] % 16 == 0 && (uintptr_t)src[i] % 16 == 0 && (nrep == 1 || (dst_stride[i] % per == 0 && src_stride[i] % per == 0));
        const long long w = a.vec[i] ? (count[i] + per - 1) / per : count[i];
        if (w > most) most = w;
    }
    a.nrep = nrep;
    const long long bz = nrep < 65535 ? nrep : 65535;
    long long bx = (most + 255) / 256;
    if (bx > 2048) bx = 2048;
    if (bx * bz > 16384) bx = 16384 / bz > 1 ? 16384 / bz : 1;   // the repetitions fill the chip; the loops cover the rest
    const dim3 grid((unsigned)bx, (unsigned)nseg, (unsigned)bz);
    trace_plain(grid, dim3(256), "segments_strided_kernel", trace_scalar<T>(), (int)sizeof(V), op != 0);
    if (op) hipLaunchKernelGGL((segments_strided_kernel<T, V, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((segments_strided_kernel<T, V, false>), grid, dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

template <typename T> int segments_launch(int op, int nseg, void* const* dst, const void* const* src, const int64_t* count, hipStream_t st) {
    typedef typename VecT<T>::v4 V4;
    constexpr int per = 16 / (int)sizeof(T);
    bool vec = true;
    long long most = 0;
    for (int i = 0; i < nseg; ++i) {
        vec = vec && count[i] % per == 0 && (uintptr_t)dst[i] % 16 == 0 && (uintptr_t)src[i] % 16 == 0;
        if (count[i] > most) most = count[i];
    }
    SegArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < nseg; ++i) { a.dst[i] = dst[i]; a.src[i] = src[i]; a.count[i] = vec ? count[i] / per : count[i]; }
    long long bx = ((vec ? most / per : most) + 255) / 256;
    if (bx < 1) bx = 1;
    if (bx > 2048) bx = 2048;
    const dim3 grid((unsigned)bx, (unsigned)nseg);
    trace_plain(grid, dim3(256), "segments_kernel", vec ? 16 : (int)sizeof(T), op != 0);
    if (sizeof(T) == 4) {
        if (vec) { if (op) hipLaunchKernelGGL((segments_kernel<V4, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((segments_kernel<V4, false>), grid, dim3(256), 0, st, a); }
        else { if (op) hipLaunchKernelGGL((segments_kernel<T, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((segments_kernel<T, false>), grid, dim3(256), 0, st, a); }
    } else {
        typedef typename VecT<T>::v2 V2;
        if (vec) { if (op) hipLaunchKernelGGL((segments_kernel<V2, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((segments_kernel<V2, false>), grid, dim3(256), 0, st, a); }
        else { if (op) hipLaunchKernelGGL((segments_kernel<T, true>), grid, dim3(256), 0, st, a); else hipLaunchKernelGGL((segments_kernel<T, false>), grid, dim3(256), 0, st, a); }
    }
    return (int)hipGetLastError();
}
}  // namespace

// z-slab, split-halo analysis: the t pass reads whole z-extended frames, so the two halo buffers (nt, ab, ny, nx) / (nt, aa, ny, nx) and
// the local slab are assembled into one (nt, ab + n + aa, ny, nx) scratch -- one strided segment launch (3 runs x nt frames) -- and the
// level runs on it
template <typename T>
static int slab_split_z_impl(ndwt_plan* p, const void* in, const void* hb, const void* ha, void* const* out, long long stride, hipStream_t s) {
    const long long ab = (long long)(p->filt[2].len / 2 - 1) * stride, aa = (long long)(p->filt[2].len / 2) * stride, n = p->dims[2];
    const long long P = p->comp * p->dims[0] * p->dims[1], nin = ab + n + aa;
    if (const int rc = p->zin.grow((size_t)(P * nin * p->dims[3]) * sizeof(T), "for the z-extended slab")) return rc;
    T* z = (T*)p->zin.ptr;
    void* dst[3];
    const void* src[3];
    int64_t cnt[3], dstr[3], sstr[3];
    int k = 0;
    if (ab) { dst[k] = z; src[k] = hb; cnt[k] = ab * P; dstr[k] = nin * P; sstr[k] = ab * P; ++k; }
    dst[k] = z + ab * P; src[k] = in; cnt[k] = n * P; dstr[k] = nin * P; sstr[k] = n * P; ++k;
    dst[k] = z + (ab + n) * P; src[k] = ha; cnt[k] = aa * P; dstr[k] = nin * P; sstr[k] = aa * P; ++k;
    const int rc = segments_strided_launch<T>(NDWT_SEG_COPY, k, dst, src, cnt, p->dims[3], dstr, sstr, s);
    if (rc != 0) return fail(NDWT_ERR_HIP, "segment kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return analysis_level<T>(p, z, (T* const*)out, stride, true, s);
}

// z-slab, zero-extended synthesis (scatter scheme): the 3-D part of both t-bands on the zero-extended z axis of every frame (the frames
// as batch items, each tested against the same [0, n)), then the periodic t pass: (nt, n + L - 1, ny, nx)
template <typename T> static int slab_ext_z_impl(ndwt_plan* p, int Lp, const void* const* in, void* out, hipStream_t s) {
    Syn4 f = {p->dims[3], p->dims[2], p->dims[2] + Lp - 1, p->dims[3]};
    f.z = kZZeroExt;
    return synthesis_4d<T>(p, Lp, (const T* const*)in, (T*)out, 1, f, kNoShrink, s);
}

extern "C" {

int ndwt_wave_filters(const char* wname, double* lo_d, double* hi_d, int* len) {
    const int K = parse_wavelet(wname);
    if (!K) return fail(NDWT_ERR_UNKNOWN_WAVELET, "Unknown Wavelet Name");
    if (!lo_d || !hi_d || !len) return fail(NDWT_ERR_INVALID_ARG, "null output pointer");
    wave_filters(K, lo_d, hi_d);
    *len = 2 * K;
    return NDWT_OK;
}

int64_t ndwt_num_bands(int ndim, int level) {
    if (ndim < 1 || ndim > NDWT_MAX_DIMS || level < 1) return -1;
    return (int64_t)(1 << ndim) + (int64_t)((1 << ndim) - 1) * (level - 1);
}

int ndwt_level_from_bands(int ndim, int64_t bands) {
    if (ndim < 1 || ndim > NDWT_MAX_DIMS) return -1;
    const int64_t nb = 1 << ndim;
    if (bands < nb || (bands - nb) % (nb - 1) != 0) return -1;
    return (int)(1 + (bands - nb) / (nb - 1));
}

static bool den3_eligible(const ndwt_plan* p, int fused_level1, int* Lp_out);
static int den3_taps(ndwt_plan* p, int Lp);
static int plan_create_impl(ndwt_plan** plan, int ndim, const int64_t* dims, long long global_outer, const char* const* wnames, int dtype,
                            int complexity, int pres_l2_norm, int dilation, int max_level, int device, int shard = -1, long long howmany = 0,
                            long long inner = 1) {
    if (!plan) return fail(NDWT_ERR_INVALID_ARG, "null plan pointer");
    *plan = nullptr;
    if (ndim < 1 || ndim > NDWT_MAX_DIMS) return fail(NDWT_ERR_INVALID_ARG, "ndim must be 1..4");
    if (!dims || !wnames) return fail(NDWT_ERR_INVALID_ARG, "null dims/wnames");
    if (dtype != NDWT_F32 && dtype != NDWT_F64) return fail(NDWT_ERR_INVALID_ARG, "dtype must be NDWT_F32 or NDWT_F64");
    if (complexity != NDWT_REAL && complexity != NDWT_COMPLEX_INTERLEAVED) return fail(NDWT_ERR_INVALID_ARG, "bad complexity");
    if (dilation != NDWT_DILATION_REFERENCE && dilation != NDWT_DILATION_ATROUS) return fail(NDWT_ERR_INVALID_ARG, "bad dilation mode");
    if (max_level < 1 || max_level > 30) return fail(NDWT_ERR_INVALID_ARG, "max_level must be 1..30");
    std::unique_ptr<ndwt_plan> owner(new ndwt_plan());    // a plan that fails below frees what it holds on the way out
    ndwt_plan* const p = owner.get();
    p->ndim = ndim;
    p->dtype = dtype;
    p->complexity = complexity;
    p->l2 = pres_l2_norm ? 1 : 0;
    p->dilation = dilation;
    p->max_level = max_level;
    p->device = device;
    p->esize = dtype == NDWT_F32 ? 4 : 8;
    p->comp = complexity == NDWT_COMPLEX_INTERLEAVED ? 2 : 1;
    p->shard = shard >= 0 ? shard : ndim - 1;
    static const char* ordn[4] = {"First", "Second", "Third", "Fourth"};
    p->howmany = howmany;
    p->inner = inner;
    p->vol = p->comp * inner * (howmany > 0 ? howmany : 1);
    for (int a = 0; a < ndim; ++a) {
        if (dims[a] < 1) return fail(NDWT_ERR_INVALID_ARG, "dims[%d] must be >= 1", a);
        const int K = parse_wavelet(wnames[a]);
        if (!K) return fail(NDWT_ERR_UNKNOWN_WAVELET, "Unknown Wavelet Name");
        p->dims[a] = dims[a];
        p->order[a] = K;
        p->filt[a] = make_axis_filter(K, p->l2 != 0);
        // nd_dwt_3D.m:277-286; for a slab plan the check is on the whole sharded axis, not on the local planes
        const long long axis_len = (a == p->shard && global_outer > 0) ? global_outer : dims[a];
        if (a == p->shard && global_outer > 0 && p->filt[a].len > dims[a]) p->thin_slab = 1;
        if (p->filt[a].len > axis_len)
            return fail(NDWT_ERR_FILTER_TOO_LONG, "%s Dimension of Data is shorter than the wavelet filter being used", ordn[a]);
        p->vol *= dims[a];
    }
    p->uniform_yz = ndim >= 3 && p->order[1] == p->order[2];   // (the same wavelet: the same taps)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(NDWT_ERR_NO_DEVICE, "no usable HIP device (requested %d of %d): this engine has no CPU path", device, ndev);
    if (hipSetDevice(device) != hipSuccess) return fail(NDWT_ERR_NO_DEVICE, "hipSetDevice(%d) failed", device);
    {
        hipDeviceProp_t prop;
        p->num_cus = (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    const int napprox = max_level >= 3 ? 2 : (max_level == 2 ? 1 : 0);
    for (int i = 0; i < napprox; ++i)
        if (const int rc = p->approx_base[i].grow((size_t)p->vol * p->esize + kApproxSkew, "of the approximation scratch", false)) return rc;
    int Lp = level_route(sel(p), 1, 0, kWholeArray).Lp;
    // a batched 1-D plan whose levels can cascade (Fwd1C / Inv1C read Taps3<T, L>, axis 0): the table of its own tap length
    if (!Lp && howmany > 0 && inner == 1 && p->filt[0].len <= 8 && (cascade1_instantiated({false, dtype == NDWT_F64, (int)p->comp, p->filt[0].len, 2}))) {
        Lp = p->filt[0].len;
        // ... and both directions in one table for the one-launch denoise (Den1C reads Taps1D<T, L>)
        const int rc = with_scalar(p, [&](auto t) {
            std::vector<decltype(t)> host;
            append_taps3(host, fused_taps(p, Lp, false), false);
            append_taps3(host, fused_taps(p, Lp, true), false);
            return p->taps_den1.upload(host.data(), host.size() * sizeof(t), "the tap table of the one-launch denoise");
        });
        if (rc) return rc;
    }
    // a plan with fused levels (the analysis side admits the most tap lengths): Taps3, and for the synthesis Taps3Y -- the same, then the
    // x tap pairs of the pair-packed kernel
    for (int inv = 0; inv < 2 && Lp; ++inv) {
        const int rc = with_scalar(p, [&](auto t) {
            std::vector<decltype(t)> host;
            append_taps3(host, fused_taps(p, Lp, inv != 0), inv != 0);
            return p->taps_dev[inv].upload(host.data(), host.size() * sizeof(t), "the tap table");
        });
        if (rc) return rc;
    }
    // the tap table of the fused level-1 denoising kernel, where that kernel can serve this plan: ndwt_denoise then only enqueues
    // (the default fused_level1 = 1 admits up to 6 taps, 2 admits 8: build for 8)
    int Lden = 0;
    if (den3_eligible(p, 2, &Lden) && den3_taps(p, Lden) != NDWT_OK) return NDWT_ERR_ALLOC;
    *plan = owner.release();
    return NDWT_OK;
}

int ndwt_plan_create(ndwt_plan** plan, int ndim, const int64_t* dims, const char* const* wnames, int dtype, int complexity,
                     int pres_l2_norm, int dilation, int max_level, int device) {
    return plan_create_impl(plan, ndim, dims, -1, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, device);
}

int ndwt_plan_create_many(ndwt_plan** plan, int ndim, const int64_t* dims, int64_t howmany, const char* const* wnames, int dtype,
                          int complexity, int pres_l2_norm, int dilation, int max_level, int device) {
    if (plan) *plan = nullptr;
    if (howmany < 1) return fail(NDWT_ERR_INVALID_ARG, "howmany must be >= 1 (got %lld)", (long long)howmany);
    if (ndim >= 2 && ndim <= NDWT_MAX_DIMS)
        return fail(NDWT_ERR_UNSUPPORTED, "batched plans are 1-D in this version: ndim = %d is not supported (loop over ndwt_plan_create plans)", ndim);
    return plan_create_impl(plan, ndim, dims, -1, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, device, -1, howmany);
}

// A transform of the leading axes only.  Everything is checked before any device call.  k filtered axes of ndim: k == ndim is
// ndwt_plan_create itself; k < ndim is the batched plan generalised -- ndim = k, howmany = the product of the axes left alone (k == 1: the
// batched 1-D plan of ndwt_plan_create_many, kernels and all).
int ndwt_plan_create_axes(ndwt_plan** plan, int ndim, const int64_t* dims, unsigned axes, const char* const* wnames, int dtype, int complexity,
                          int pres_l2_norm, int dilation, int max_level, int device) {
    if (plan) *plan = nullptr;
    if (ndim < 1 || ndim > NDWT_MAX_DIMS) return fail(NDWT_ERR_INVALID_ARG, "ndim must be 1..4");
    if (axes == 0 || (axes >> ndim) != 0)
        return fail(NDWT_ERR_INVALID_ARG, "axes mask 0x%x: it must name at least one of the %d axes and none beyond them", axes, ndim);
    int k = 0;
    while ((axes >> k) & 1u) ++k;
    if ((axes >> k) != 0)
        return fail(NDWT_ERR_UNSUPPORTED, "axes mask 0x%x is not supported: this version filters leading axes only (masks 0x1, 0x3, 0x7, 0xf)", axes);
    if (k == ndim) return plan_create_impl(plan, ndim, dims, -1, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, device);
    if (!dims || !wnames) return fail(NDWT_ERR_INVALID_ARG, "null dims/wnames");
    long long items = 1;
    for (int a = k; a < ndim; ++a) {
        if (dims[a] < 1) return fail(NDWT_ERR_INVALID_ARG, "dims[%d] must be >= 1", a);
        if (dims[a] > (1LL << 40) / items) return fail(NDWT_ERR_INVALID_ARG, "the axes left alone hold more than 2^40 items");
        items *= dims[a];
    }
    return plan_create_impl(plan, k, dims, -1, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, device, -1, items);
}

// Samples of `inner` elements that lie together: the array is [inner, dims.., howmany], every filtered axis strided.  Everything is
// checked before any device call.  inner == 1 is the plan ndwt_plan_create_axes makes for [dims.., howmany] with its leading axes filtered
// (the same plan fields, so the same routes and the same bits); the plan is always a batched one (howmany >= 1).
int ndwt_plan_create_interleaved(ndwt_plan** plan, int ndim, const int64_t* dims, int64_t inner, int64_t howmany, const char* const* wnames,
                                 int dtype, int complexity, int pres_l2_norm, int dilation, int max_level, int device) {
    if (plan) *plan = nullptr;
    if (ndim < 1 || ndim > NDWT_MAX_DIMS) return fail(NDWT_ERR_INVALID_ARG, "ndim must be 1..4 (got %d)", ndim);
    if (inner < 1) return fail(NDWT_ERR_INVALID_ARG, "inner must be >= 1 (got %lld)", (long long)inner);
    if (howmany < 1) return fail(NDWT_ERR_INVALID_ARG, "howmany must be >= 1 (got %lld)", (long long)howmany);
    if (inner > (1LL << 40) || howmany > (1LL << 40)) return fail(NDWT_ERR_INVALID_ARG, "inner and howmany are at most 2^40 each");
    return plan_create_impl(plan, ndim, dims, -1, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, device, -1, howmany, inner);
}

int ndwt_plan_create_slab(ndwt_plan** plan, int ndim, const int64_t* dims_local, int64_t global_outer, const char* const* wnames,
                          int dtype, int complexity, int pres_l2_norm, int dilation, int max_level, int device) {
    if (ndim >= 1 && ndim <= NDWT_MAX_DIMS && dims_local && global_outer < dims_local[ndim - 1])
        return fail(NDWT_ERR_INVALID_ARG, "global_outer (%lld) is shorter than the local slab (%lld)", (long long)global_outer,
                    (long long)dims_local[ndim - 1]);
    return plan_create_impl(plan, ndim, dims_local, global_outer, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, device);
}

int ndwt_plan_create_slab_axis(ndwt_plan** plan, int ndim, const int64_t* dims_local, int shard_axis, int64_t global_len,
                               const char* const* wnames, int dtype, int complexity, int pres_l2_norm, int dilation, int max_level, int device) {
    if (plan) *plan = nullptr;
    if (ndim < 1 || ndim > NDWT_MAX_DIMS || !dims_local) return fail(NDWT_ERR_INVALID_ARG, "ndim must be 1..4, dims non-null");
    if (shard_axis == ndim - 1)
        return ndwt_plan_create_slab(plan, ndim, dims_local, global_len, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, device);
    if (!(ndim == 4 && shard_axis == 2))
        return fail(NDWT_ERR_UNSUPPORTED, "shard_axis %d of a %d-D volume: slab plans shard the outermost axis (%d), or z (2) of a 4-D volume",
                    shard_axis, ndim, ndim - 1);
    if (global_len < dims_local[shard_axis])
        return fail(NDWT_ERR_INVALID_ARG, "global_len (%lld) is shorter than the local slab (%lld)", (long long)global_len,
                    (long long)dims_local[shard_axis]);
    return plan_create_impl(plan, ndim, dims_local, global_len, wnames, dtype, complexity, pres_l2_norm, dilation, max_level, device, shard_axis);
}

int ndwt_plan_destroy(ndwt_plan* p) {
    if (!p) return NDWT_OK;
    if (p->live_coefs > 0)                                // (a handle points back at its plan: release the handles first)
        return fail(NDWT_ERR_INVALID_ARG, "%d coefficient handle(s) of this plan are still alive: ndwt_coef_release them first", p->live_coefs);
    (void)hipSetDevice(p->device);
    delete p;
    return NDWT_OK;
}

int ndwt_plan_set_profiling(ndwt_plan* p, int enable) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    p->profiling = enable ? 1 : 0;
    return NDWT_OK;
}

// sums (and clears) the event records of one kernel kind; synchronises the device
int ndwt_plan_get_profile(ndwt_plan* p, int kind, double* total_ms, int64_t* launches) {
    if (!p || !total_ms || !launches) return fail(NDWT_ERR_INVALID_ARG, "bad arguments");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    double tot = 0;
    int64_t n = 0;
    std::vector<ProfRec> keep;
    for (auto& r : p->prof) {
        if (r.kind != kind) { keep.push_back(r); continue; }
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) { tot += ms; ++n; }
        p->ev_pool.push_back(r.start);
        p->ev_pool.push_back(r.stop);
    }
    p->prof.swap(keep);
    *total_ms = tot;
    *launches = n;
    return NDWT_OK;
}

int ndwt_plan_set_path(ndwt_plan* p, int path) {
    if (!p || (path != NDWT_PATH_AUTO && path != NDWT_PATH_GENERIC)) return fail(NDWT_ERR_INVALID_ARG, "bad plan/path");
    p->path = path;
    return NDWT_OK;
}

// test/tuning hook: grid sizing of the fused kernels (0 = default)
int ndwt_plan_set_tuning(ndwt_plan* p, int target_blocks, int force_zchunk) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    p->target_blocks = target_blocks > 0 ? target_blocks : 0;
    p->force_zchunk = force_zchunk > 0 ? force_zchunk : 0;
    return NDWT_OK;
}

// test/tuning hook (tools/: interleaved A/B runs): kernel variants and per-direction march chunks of the fused kernels; every
// variant computes the same values.  A negative argument leaves that setting as it is.  Nothing in the library reads the
// environment: a plan behaves the same whatever the caller's process has exported.
int ndwt_plan_set_variant(ndwt_plan* p, int variant_fwd, int variant_inv, int zchunk_fwd, int zchunk_inv, int fp64_fused) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    if (variant_fwd >= 0) p->variant_fwd = variant_fwd;
    if (variant_inv >= 0) p->variant_inv = variant_inv;
    if (zchunk_fwd >= 0) p->zchunk_dir[0] = zchunk_fwd;
    if (zchunk_inv >= 0) p->zchunk_dir[1] = zchunk_inv;
    if (fp64_fused >= 0) p->fp64_fused = fp64_fused ? 1 : 0;
    return NDWT_OK;
}

// test / tuning hook: 0 = ndwt_denoise materialises the level-1 detail bands (dec, thresholding in the synthesis loads, rec);
// 1 (default) = the fused level-1 kernel where it is the faster path (tap lengths <= 6); 2 = wherever it exists (8 taps too)
int ndwt_plan_set_fused_level1(ndwt_plan* p, int enable) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    p->fused_level1 = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return NDWT_OK;
}

int ndwt_plan_describe(const ndwt_plan* p, char* buf, int buflen) {
    if (!p || !buf || buflen < 1) return fail(NDWT_ERR_INVALID_ARG, "bad arguments");
    const char* s = "axis";
    const LevelRouteKind ra = level_route(sel(p), 1, 0, kWholeArray).kind, rs = level_route(sel(p), 1, 1, kWholeArray).kind;
    const bool f3a = route_fused3(ra), f3s = route_fused3(rs);
    if (f3a && f3s) s = p->ndim == 3 ? "fused3d" : "axis+fused3d";
    else if (f3a) s = p->ndim == 3 ? "fused3d analysis, axis synthesis" : "axis+fused3d analysis, axis synthesis";
    else if (ra == kRouteFused2) s = "fused2d";
    int L1 = 0;
    if (p->howmany > 0) s = cascade1_levels(sel(p), false, 2, &L1) ? "batched1d cascade" : "batched1d axis";
    if (p->howmany > 0 && p->ndim >= 2) {                 // a stack (ndwt_plan_create_axes): what two levels of it run today
        int Lp = 0;
        s = cascade2_levels(sel(p), false, 2, &Lp) ? "stack2d cascade" : ra == kRouteFused2 ? "stack2d fused" : f3a ? "stack3d fused" : "stack axis";
    }
    if (p->inner > 1) {                                   // interleaved samples (ndwt_plan_create_interleaved): what two levels of it run today
        int Lm = 0;
        s = cascadem_levels(sel(p), false, 2, &Lm) ? "interleaved cascade" : "interleaved axis";
    }
    snprintf(buf, (size_t)buflen, "%s", s);
    return NDWT_OK;
}

// band pitch in elements -> scalars; 0 = packed
static int pitch_scalars(const ndwt_plan* p, int64_t band_pitch, long long* bs) {
    *bs = band_pitch == 0 ? p->vol : (long long)band_pitch * p->comp;
    if (*bs < p->vol) return fail(NDWT_ERR_INVALID_ARG, "band pitch %lld is smaller than a band (%lld elements)", (long long)band_pitch, p->vol / p->comp);
    return NDWT_OK;
}

int ndwt_dec_pitched(ndwt_plan* p, const void* x, void* y, int64_t band_pitch, int level, void* stream) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!x || !y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return dec_impl(p, (const decltype(t)*)x, (decltype(t)*)y, bs, level, (hipStream_t)stream); });
}

int ndwt_rec_pitched(ndwt_plan* p, const void* y, int64_t band_pitch, void* x, int level, void* stream) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!x || !y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return rec_impl(p, (const decltype(t)*)y, bs, (decltype(t)*)x, level, kNoShrink, (hipStream_t)stream); });
}

int ndwt_dec(ndwt_plan* p, const void* x, void* y, int level, void* stream) { return ndwt_dec_pitched(p, x, y, 0, level, stream); }
int ndwt_rec(ndwt_plan* p, const void* y, void* x, int level, void* stream) { return ndwt_rec_pitched(p, y, 0, x, level, stream); }

int64_t ndwt_band_pitch(const ndwt_plan* p) {
    if (!p) return 0;
    const long long skew = 256 / (long long)(p->esize * p->comp);   // 256 bytes, in elements
    return p->vol / p->comp + (skew > 0 ? skew : 1);
}

// Device staging of the host-pointer forms, owned by the plan and grown on demand: the gateway calls dec / rec with one configuration
// thousands of times (README.md:2), and a hipMalloc + hipFree of the 12 GB a 512^3 3-level transform stages costs milliseconds per call.
static int ensure_stage(ndwt_plan* p, int which, size_t bytes) { return p->stage[which].grow(bytes, "of the staging buffer"); }

static int host_roundtrip(ndwt_plan* p, bool inverse, const void* src, void* dst, int level) {
    int rc = refuse_batched(p, "a host-pointer transform");
    if (rc) return rc;
    rc = check_level(p, level);
    if (rc) return rc;
    if (!src || !dst) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    HIP_TRY(hipSetDevice(p->device));
    const size_t bx = (size_t)p->vol * p->esize;
    const size_t by = bx * (size_t)ndwt_num_bands(p->ndim, level);
    rc = ensure_stage(p, 0, bx);
    if (rc == NDWT_OK) rc = ensure_stage(p, 1, by);
    if (rc) return rc;
    void *dx = p->stage[0].ptr, *dy = p->stage[1].ptr;
    hipError_t e = hipMemcpy(inverse ? dy : dx, src, inverse ? by : bx, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = inverse ? ndwt_rec(p, dy, dx, level, nullptr) : ndwt_dec(p, dx, dy, level, nullptr);
        if (rc == NDWT_OK) e = hipMemcpy(dst, inverse ? dx : dy, inverse ? bx : by, hipMemcpyDeviceToHost);
    }
    if (rc) return rc;
    if (e != hipSuccess) return fail(NDWT_ERR_HIP, "staging copy failed: %s", hipGetErrorString(e));
    return NDWT_OK;
}

int ndwt_plan_release_staging(ndwt_plan* p) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    p->stage[0].reset();
    p->stage[1].reset();
    return NDWT_OK;
}

// ---- device-resident coefficients (include/ndwt.h: ndwt_coef_*) ----
struct ndwt_coef {
    ndwt_plan* plan;
    int level;
    long long bands;
    long long pitch;                   // elements between bands (ndwt_band_pitch)
    DevBuf dev;
};

static int coef_check(const ndwt_plan* p, const ndwt_coef* c) {
    if (const int rc = refuse_batched(p, "a coefficient handle")) return rc;
    if (!p || !c) return fail(NDWT_ERR_INVALID_ARG, "null plan / coefficient handle");
    if (c->plan != p) return fail(NDWT_ERR_INVALID_ARG, "this coefficient handle belongs to another plan");
    return NDWT_OK;
}

int ndwt_coef_create(ndwt_plan* p, int level, ndwt_coef** out) {
    int rc = refuse_batched(p, "a coefficient handle");
    if (rc) return rc;
    rc = check_level(p, level);
    if (rc) return rc;
    if (!out) return fail(NDWT_ERR_INVALID_ARG, "null output pointer");
    HIP_TRY(hipSetDevice(p->device));
    std::unique_ptr<ndwt_coef> c(new ndwt_coef());
    c->plan = p;
    c->level = level;
    c->bands = ndwt_num_bands(p->ndim, level);
    c->pitch = ndwt_band_pitch(p);
    if (const int rc = c->dev.grow((size_t)c->bands * (size_t)c->pitch * (size_t)p->comp * p->esize, "of a coefficient set")) return rc;
    p->live_coefs++;
    *out = c.release();
    return NDWT_OK;
}

int ndwt_coef_release(ndwt_coef* c) {
    if (!c) return NDWT_OK;
    (void)hipSetDevice(c->plan->device);
    (void)hipDeviceSynchronize();
    c->plan->live_coefs--;
    delete c;
    return NDWT_OK;
}

int ndwt_coef_info(const ndwt_coef* c, int* level, int64_t* bands, int64_t* band_pitch, void** dev_ptr) {
    if (!c) return fail(NDWT_ERR_INVALID_ARG, "null coefficient handle");
    if (level) *level = c->level;
    if (bands) *bands = c->bands;
    if (band_pitch) *band_pitch = c->pitch;
    if (dev_ptr) *dev_ptr = c->dev.ptr;
    return NDWT_OK;
}

// The handle an upload fills, after the checks both uploads make: *coef where the caller passes one of this plan and level for reuse, else
// a new one.  `fill` writes its coefficients; where that fails, a handle made here is released and *coef stays as it was.
extern "C++" template <class F> static int coef_upload(ndwt_plan* p, int level, const void* host, ndwt_coef** coef, F&& fill) {
    int rc = refuse_batched(p, "a coefficient handle");
    if (rc) return rc;
    rc = check_level(p, level);
    if (rc) return rc;
    if (!host || !coef) return fail(NDWT_ERR_INVALID_ARG, "null pointer");
    HIP_TRY(hipSetDevice(p->device));
    ndwt_coef* c = *coef;
    if (c && (c->plan != p || c->level != level)) return fail(NDWT_ERR_INVALID_ARG, "the handle passed for reuse holds another plan's / level's coefficients");
    const bool fresh = c == nullptr;
    if (fresh) {
        rc = ndwt_coef_create(p, level, &c);
        if (rc) return rc;
    }
    rc = fill(c);
    if (rc) {
        if (fresh) ndwt_coef_release(c);
        return rc;
    }
    *coef = c;
    return NDWT_OK;
}

// x (host) -> coefficients that STAY on the device: only the signal crosses PCIe (0.5 GB instead of 12.3 GB at 512^3, 3 levels)
int ndwt_coef_dec_host(ndwt_plan* p, const void* x_host, int level, ndwt_coef** coef) {
    return coef_upload(p, level, x_host, coef, [&](ndwt_coef* c) {
        const size_t bx = (size_t)p->vol * p->esize;
        int rc = ensure_stage(p, 0, bx);
        if (rc) return rc;
        hipError_t e = hipMemcpy(p->stage[0].ptr, x_host, bx, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            rc = ndwt_dec_pitched(p, p->stage[0].ptr, c->dev.ptr, c->pitch, level, nullptr);
            if (rc) return rc;
            e = hipStreamSynchronize(nullptr);
        }
        return e == hipSuccess ? NDWT_OK : fail(NDWT_ERR_HIP, "staging copy failed: %s", hipGetErrorString(e));
    });
}

int ndwt_coef_rec_host(ndwt_plan* p, const ndwt_coef* c, void* x_host) {
    int rc = coef_check(p, c);
    if (rc) return rc;
    if (!x_host) return fail(NDWT_ERR_INVALID_ARG, "null pointer");
    HIP_TRY(hipSetDevice(p->device));
    const size_t bx = (size_t)p->vol * p->esize;
    rc = ensure_stage(p, 0, bx);
    if (rc) return rc;
    rc = ndwt_rec_pitched(p, c->dev.ptr, c->pitch, p->stage[0].ptr, c->level, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(x_host, p->stage[0].ptr, bx, hipMemcpyDeviceToHost));
    return NDWT_OK;
}

int ndwt_coef_shrink(ndwt_plan* p, ndwt_coef* c, double threshold, int mode) {
    int rc = coef_check(p, c);
    if (rc) return rc;
    rc = ndwt_shrink_pitched(p, c->dev.ptr, c->pitch, c->level, threshold, mode, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NDWT_OK;
}

// the coefficients in the reference's packed layout (band axis last, nd_dwt_mex.c:83) to / from host memory
int ndwt_coef_get_host(ndwt_plan* p, const ndwt_coef* c, void* y_host) {
    int rc = coef_check(p, c);
    if (rc) return rc;
    if (!y_host) return fail(NDWT_ERR_INVALID_ARG, "null pointer");
    HIP_TRY(hipSetDevice(p->device));
    const size_t band = (size_t)p->vol * p->esize, pitch = (size_t)c->pitch * (size_t)p->comp * p->esize;
    HIP_TRY(hipMemcpy2D(y_host, band, c->dev.ptr, pitch, band, (size_t)c->bands, hipMemcpyDeviceToHost));
    return NDWT_OK;
}

int ndwt_coef_put_host(ndwt_plan* p, int level, const void* y_host, ndwt_coef** coef) {
    return coef_upload(p, level, y_host, coef, [&](ndwt_coef* c) {
        const size_t band = (size_t)p->vol * p->esize, pitch = (size_t)c->pitch * (size_t)p->comp * p->esize;
        const hipError_t e = hipMemcpy2D(c->dev.ptr, pitch, y_host, band, band, (size_t)c->bands, hipMemcpyHostToDevice);
        return e == hipSuccess ? NDWT_OK : fail(NDWT_ERR_HIP, "upload of the coefficients failed: %s", hipGetErrorString(e));
    });
}

int ndwt_dec_host(ndwt_plan* p, const void* x, void* y, int level) { return host_roundtrip(p, false, x, y, level); }
int ndwt_rec_host(ndwt_plan* p, const void* y, void* x, int level) { return host_roundtrip(p, true, y, x, level); }

// ---- consumers for iterative solvers (not in the reference: its users threshold in MATLAB) ----
static int shrink_check(const ndwt_plan* p, int level, double thr, int mode) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!(thr >= 0.0)) return fail(NDWT_ERR_INVALID_ARG, "threshold must be >= 0");
    if (mode != NDWT_SHRINK_SOFT && mode != NDWT_SHRINK_HARD) return fail(NDWT_ERR_INVALID_ARG, "mode must be NDWT_SHRINK_SOFT or NDWT_SHRINK_HARD");
    return NDWT_OK;
}

int ndwt_shrink_pitched(ndwt_plan* p, void* y, int64_t band_pitch, int level, double threshold, int mode, void* stream) {
    int rc = shrink_check(p, level, threshold, mode);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return shrink_impl(p, (decltype(t)*)y, bs, level, threshold, mode, (hipStream_t)stream); });
}
int ndwt_shrink(ndwt_plan* p, void* y, int level, double threshold, int mode, void* stream) {
    return ndwt_shrink_pitched(p, y, 0, level, threshold, mode, stream);
}

// ---- one threshold per band (include/ndwt.h: ndwt_band_gains says what to scale them by) ----
static int bands_check(const ndwt_plan* p, int level, const double* thr, int mode) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!thr) return fail(NDWT_ERR_INVALID_ARG, "null thresholds");
    const long long nb = ndwt_num_bands(p->ndim, level);
    for (long long b = 0; b < nb; ++b)
        if (!(thr[b] >= 0.0)) return fail(NDWT_ERR_INVALID_ARG, "threshold of band %lld must be >= 0", b);
    if (mode != NDWT_SHRINK_SOFT && mode != NDWT_SHRINK_HARD) return fail(NDWT_ERR_INVALID_ARG, "mode must be NDWT_SHRINK_SOFT or NDWT_SHRINK_HARD");
    return NDWT_OK;
}
// one run of shrink_kernel per band with a non-zero threshold, band 0 like any other; a zero leaves its band untouched (no launch)
extern "C++" template <typename T> static int shrink_bands_impl(ndwt_plan* p, T* y, long long bs, int level, const double* thr, int mode, hipStream_t s) {
    const long long nb = ndwt_num_bands(p->ndim, level);
    for (long long b = 0; b < nb; ++b) {
        if (thr[b] == 0.0) continue;
        const int rc = shrink_run<T>(p, y + b * bs, p->vol, thr[b], mode, s);
        if (rc) return rc;
    }
    return NDWT_OK;
}

int ndwt_shrink_bands(ndwt_plan* p, void* y, int64_t band_pitch, int level, const double* thresholds, int mode, void* stream) {
    int rc = bands_check(p, level, thresholds, mode);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return shrink_bands_impl(p, (decltype(t)*)y, bs, level, thresholds, mode, (hipStream_t)stream); });
}

// Periodic dec of a unit impulse, axis by axis: A[l] / D[l] = the l2 norm of the approximation / detail response of level l on an axis of
// n samples -- the periodised convolution of the levels' taps at their tap strides.  A band of a k-D transform is the outer product of
// its axes' responses, so its norm is the product of theirs.
static void axis_gains(const AxisFilter& f, long long n, bool atrous, int level, double* A, double* D) {
    std::vector<double> cur((size_t)n, 0.0), lo((size_t)n), hi((size_t)n);
    cur[0] = 1.0;
    A[0] = 1.0;
    D[0] = 0.0;
    for (int lev = 1; lev <= level; ++lev) {
        const long long stride = atrous ? (1LL << (lev - 1)) % n : 1LL;
        double sl = 0.0, sh = 0.0;
        for (long long i = 0; i < n; ++i) {
            double al = 0.0, ah = 0.0;
            long long pos = i;
            for (int j = 0; j < f.len; ++j) {
                al += f.ana_lo[j] * cur[(size_t)pos];
                ah += f.ana_hi[j] * cur[(size_t)pos];
                pos += stride;
                if (pos >= n) pos -= n;
            }
            lo[(size_t)i] = al;
            hi[(size_t)i] = ah;
            sl += al * al;
            sh += ah * ah;
        }
        A[lev] = std::sqrt(sl);
        D[lev] = std::sqrt(sh);
        cur.swap(lo);
    }
}

int ndwt_band_gains(int ndim, const int64_t* dims, const char* const* wnames, int pres_l2_norm, int dilation, int level, double* gains) {
    if (ndim < 1 || ndim > NDWT_MAX_DIMS) return fail(NDWT_ERR_INVALID_ARG, "ndim must be 1..4");
    if (!dims || !wnames) return fail(NDWT_ERR_INVALID_ARG, "null dims/wnames");
    if (!gains) return fail(NDWT_ERR_INVALID_ARG, "null output pointer");
    if (dilation != NDWT_DILATION_REFERENCE && dilation != NDWT_DILATION_ATROUS) return fail(NDWT_ERR_INVALID_ARG, "bad dilation mode");
    if (level < 1 || level > 30) return fail(NDWT_ERR_INVALID_ARG, "level must be 1..30");
    static const char* ordn[4] = {"First", "Second", "Third", "Fourth"};
    std::vector<double> A[NDWT_MAX_DIMS], D[NDWT_MAX_DIMS];
    for (int a = 0; a < ndim; ++a) {
        if (dims[a] < 1) return fail(NDWT_ERR_INVALID_ARG, "dims[%d] must be >= 1", a);
        const int K = parse_wavelet(wnames[a]);
        if (!K) return fail(NDWT_ERR_UNKNOWN_WAVELET, "Unknown Wavelet Name");
        const AxisFilter f = make_axis_filter(K, pres_l2_norm != 0);
        if (f.len > dims[a]) return fail(NDWT_ERR_FILTER_TOO_LONG, "%s Dimension of Data is shorter than the wavelet filter being used", ordn[a]);
        A[a].resize((size_t)level + 1);
        D[a].resize((size_t)level + 1);
        axis_gains(f, dims[a], dilation == NDWT_DILATION_ATROUS, level, A[a].data(), D[a].data());
    }
    const int nb = 1 << ndim;
    const long long bands = ndwt_num_bands(ndim, level);
    for (long long b = 0; b < bands; ++b) {
        const int lev = b == 0 ? level : level - (int)((b - 1) / (nb - 1));     // band 0: the approximation of the last level
        const int bits = b == 0 ? 0 : 1 + (int)((b - 1) % (nb - 1));            // bit a: high-pass on axis a
        double g = 1.0;
        for (int a = 0; a < ndim; ++a) g *= ((bits >> a) & 1) ? D[a][(size_t)lev] : A[a][(size_t)lev];
        gains[b] = g;
    }
    return NDWT_OK;
}

// ---- level 1 of a denoising step without its detail bands in memory (Den3, ndwt_device.h) ----
// Float, real, 3-D, reference dilation, the same tap length L <= 8 on every axis, rows of whole 16-byte groups.
// fused_level1: the setting asked about (ndwt_plan_set_fused_level1: the plan's own for a call, 2 for "does the kernel exist for this plan")
static bool den3_eligible(const ndwt_plan* p, int fused_level1, int* Lp_out) {
    if (!fused_level1 || p->dtype != NDWT_F32 || p->complexity != NDWT_REAL || p->ndim != 3 || p->dilation != NDWT_DILATION_REFERENCE)
        return false;
    if (p->howmany > 0) return false;                     // a stack: Den3 knows one volume (its level 1 materialises like the others)
    const LevelRoute r = level_route(sel(p), 1, -1, kWholeArray);
    const int Lp = r.Lp;
    // measured, 512^3, 3 levels, ndwt_denoise with / without the fused level 1: db1 4.49 / 5.27 ms, db2 5.10 / 5.67, db3 5.72 / 6.09,
    // db4 6.30 / 6.13 -- with 8 taps the recomputation (2.3x the arithmetic of the synthesis kernel, 67 % VALU-busy) costs more than the
    // 13 volume transfers it removes, so 8 taps take the kernel only when asked to (ndwt_plan_set_fused_level1(plan, 2))
    if (r.kind != kRouteFused3 || Lp > (fused_level1 >= 2 ? 8 : 6) || !inv3y_plan_ok(sel(p), Lp)) return false;
    for (int ax = 0; ax < 3; ++ax)
        if (p->filt[ax].len != Lp) return false;
    if (p->dims[0] % 4 != 0) return false;
    *Lp_out = Lp;
    return true;
}

static int den3_taps(ndwt_plan* p, int Lp) {
    if (p->taps_den.ptr) return NDWT_OK;
    std::vector<float> h;                                 // TapsDen<float, Lp>
    if (!build_taps_den(h, fused_taps(p, Lp, true), fused_taps(p, Lp, false)))
        return fail(NDWT_ERR_UNSUPPORTED, "internal: analysis taps are not a mirrored pair");
    return p->taps_den.upload(h.data(), h.size() * sizeof(float), "the tap table of the fused level-1 kernel");
}

// kind 0: approximation band of one analysis level (x -> out);  kind 1: Den3 (x, approximation -> out), thresholding as `shrink` says
static int den3_launch(ndwt_plan* p, int kind, int Lp, const float* x, const float* apx, float* out, const ShrinkOnLoad& shrink, hipStream_t s) {
    Fused3Args<float> a;
    memset(&a, 0, sizeof a);
    a.n1 = (int)p->dims[0]; a.n2 = (int)p->dims[1]; a.n3 = (int)p->dims[2];
    a.nbatch = 1;
    a.z_wrap = 1;
    a.in[0] = x; a.in[1] = apx;
    a.out[0] = out;
    a.in_bstride = a.out_bstride = p->vol;
    if (kind == 1) {
        a.shrink_thr = (float)shrink.thr;
        a.shrink_mask = 0xFE;
        a.shrink_hard = shrink.mode == 2;
    }
    // one workgroup per CU (1024 threads); Den3's march starts 2 (L - 1) planes before its first output plane
    const bool small_tile = kind == 0 && p->variant_fwd != kFwdTall && a.n2 > 16;   // the band-0 analysis on 64 x 16 tiles, 3 workgroups per CU (0.36 vs 0.42 ms; kFwdTall: A/B)
    if (small_tile) fused3_geometry(a, 64, 16, Lp, p->target_blocks > 0 ? p->target_blocks : p->num_cus * 3, p->force_zchunk);
    else fused3_geometry(a, 64, 32, kind == 1 ? 2 * Lp - 1 : Lp, p->target_blocks > 0 ? p->target_blocks : p->num_cus, p->force_zchunk);
    float* outs[1] = {out};
    a.nt = nt_store_ok<float>(a.rs, a.plane, p->vol, outs, 1);
    prof_begin(p, kind == 1 ? NDWT_KERNEL_FUSED_SYNTHESIS : NDWT_KERNEL_FUSED_ANALYSIS, s);
    const bool vec4 = aligned_vec4<float>(x) && aligned_vec4<float>(out);
    int rc = kind == 1 ? launch_den3_f32(a, Lp, p->taps_den.ptr, s) : launch_fwd3_low_f32(a, Lp, vec4, small_tile ? 0 : 2, p->taps_dev[0].ptr, s);
    prof_end(p, s, rc);
    if (rc == -1) return fail(NDWT_ERR_UNSUPPORTED, "fused level-1 kernel not instantiated for tap length %d", Lp);
    if (rc == -2) return fail(NDWT_ERR_UNSUPPORTED, "internal: launch geometry does not match the level-1 kernel's tile");
    if (rc != 0) return fail(NDWT_ERR_HIP, "fused level-1 kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return NDWT_OK;
}

// The plan's coefficient scratch, grown for `level` levels, and the transform of x in it.  The bands are pitched (ndwt_band_pitch): nobody
// else reads them.  *bs: the distance between them in scalars
extern "C++" template <typename T> static int dec_scratch(ndwt_plan* p, const T* x, int level, hipStream_t s, T** coef, long long* bs) {
    *bs = (long long)ndwt_band_pitch(p) * p->comp;
    const int rc = p->coef.grow((size_t)*bs * p->esize * (size_t)ndwt_num_bands(p->ndim, level), "for the coefficient scratch");
    if (rc) return rc;
    *coef = (T*)p->coef.ptr;
    return dec_impl<T>(p, x, *coef, *bs, level, s);
}

// dec -> shrink -> rec with level 1 fused: x -> approximation of level 1 (band 0 only) -> levels 2 .. `level` as a (level - 1)-level
// transform of that band (the reference applies the same filters at every level, nd_dwt_3D.m:178-186) with the thresholding in the
// synthesis kernels' loads -> Den3(x, reconstructed approximation).  Volumes moved at level 1: 5 instead of 18.
static int denoise_fused_level1(ndwt_plan* p, int Lp, const float* x, float* out, int level, const ShrinkOnLoad& shrink, hipStream_t s) {
    int rc = den3_taps(p, Lp);
    if (rc) return rc;
    rc = p->den_a1.grow((size_t)p->vol * sizeof(float) + kApproxSkew, "of the level-1 approximation scratch", false);
    if (rc) return rc;
    float* a1 = (float*)((char*)p->den_a1.ptr + kApproxSkew);   // level-1 approximation, then its reconstruction (256 B off the alignment, like the ping-pong scratch)
    rc = den3_launch(p, 0, Lp, x, nullptr, a1, kNoShrink, s);
    if (rc == NDWT_OK && level > 1) {
        float* coef = nullptr;                            // (a float 3-D plan: pitch * esize * ndwt_num_bands(3, level - 1) bytes)
        long long bs = 0;
        rc = dec_scratch<float>(p, a1, level - 1, s, &coef, &bs);
        if (rc == NDWT_OK) rc = rec_impl<float>(p, coef, bs, a1, level - 1, shrink, s);   // (thresholding in the band loads)
    }
    if (rc == NDWT_OK) rc = den3_launch(p, 1, Lp, x, a1, out, shrink, s);
    return rc;
}

int ndwt_denoise(ndwt_plan* p, const void* x, void* out, int level, double threshold, int mode, void* stream) {
    int rc = shrink_check(p, level, threshold, mode);
    if (rc) return rc;
    if (!x || !out) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    const ShrinkOnLoad shrink = shrink_on_load(threshold, mode);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(p->device));
    {
        // the finest level without its detail bands in memory, where the fused level-1 kernel applies (it reads x around every
        // output voxel while other workgroups write `out`: not in place)
        int Lp1 = 0;
        const char *xb = (const char*)x, *ob = (const char*)out;
        const size_t nbytes = (size_t)p->vol * p->esize;
        const bool disjoint = xb + nbytes <= ob || ob + nbytes <= xb;
        if (den3_eligible(p, p->fused_level1, &Lp1) && disjoint && aligned_vec4<float>(x) && aligned_vec4<float>(out))
            return denoise_fused_level1(p, Lp1, (const float*)x, (float*)out, level, shrink, s);
    }
    return with_scalar(p, [&](auto t) {
        typedef decltype(t) T;
        T* coef = nullptr;
        long long bs = 0;
        int rc = dec_scratch<T>(p, (const T*)x, level, s, &coef, &bs);
        if (rc) return rc;
        // every level is reconstructed by a lane-shift kernel: the detail bands are thresholded in registers as that
        // kernel loads them, and the separate pass (a read and a write of every detail band) disappears
        if (fused_shrink_capable(sel(p))) return rec_impl<T>(p, coef, bs, (T*)out, level, shrink, s);
        rc = shrink_impl<T>(p, coef, bs, level, threshold, mode, s);
        if (rc == NDWT_OK) rc = rec_impl<T>(p, coef, bs, (T*)out, level, kNoShrink, s);
        return rc;
    });
}

int ndwt_denoise_bands(ndwt_plan* p, const void* x, void* out, int level, const double* thresholds, int mode, void* stream) {
    int rc = bands_check(p, level, thresholds, mode);
    if (rc) return rc;
    if (!x || !out) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    HIP_TRY(hipSetDevice(p->device));
    {
        // a batched 1-D plan: the whole depth in one launch, where that exists and is wanted (denoise1_levels / denoise1_wanted)
        const SelPlan sp = sel(p);
        const int n = denoise1_wanted(sp) ? denoise1_levels(sp, level) : 0;
        if (n) {
            rc = with_scalar(p, [&](auto t) {
                return denoise1_run<decltype(t)>(p, p->filt[0].len, n, (const decltype(t)*)x, (decltype(t)*)out, thresholds, mode, (hipStream_t)stream);
            });
            if (rc != -1) return rc;                      // -1: not this data -- the general route, silently
        }
    }
    // the general route: dec into the plan's pitched scratch, one shrink pass per band, rec (no thresholding in the synthesis loads)
    return with_scalar(p, [&](auto t) {
        typedef decltype(t) T;
        T* coef = nullptr;
        long long bs = 0;
        int rc = dec_scratch<T>(p, (const T*)x, level, (hipStream_t)stream, &coef, &bs);
        if (rc == NDWT_OK) rc = shrink_bands_impl<T>(p, coef, bs, level, thresholds, mode, (hipStream_t)stream);
        if (rc == NDWT_OK) rc = rec_impl<T>(p, coef, bs, (T*)out, level, kNoShrink, (hipStream_t)stream);
        return rc;
    });
}

// ---- order statistics of a band's |c|, and the noise estimate on top of them (include/ndwt.h; the kernels: ndwt_device_select.h) ----
// what is decided without a device: the arguments, and the band's size against the 32-bit counters
static int select_check(const ndwt_plan* p, const void* y, int level, int64_t band, int nk, const int64_t* k, const double* values) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    if (!k) return fail(NDWT_ERR_INVALID_ARG, "null rank array (k)");
    if (!values) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (values)");
    const long long nb = ndwt_num_bands(p->ndim, level), N = p->vol / p->comp;
    if (band < 0 || band >= nb) return fail(NDWT_ERR_INVALID_ARG, "band %lld outside 0..%lld of a level-%d coefficient array", (long long)band, nb - 1, level);
    if (nk < 1 || nk > kSelectMaxRanks) return fail(NDWT_ERR_INVALID_ARG, "nk = %d: 1..%d ranks per call", nk, kSelectMaxRanks);
    for (int i = 0; i < nk; ++i)
        if (k[i] < 0 || k[i] >= N) return fail(NDWT_ERR_INVALID_ARG, "k[%d] = %lld outside [0, %lld), the elements of a band", i, (long long)k[i], N);
    if (!select_fits(N)) return fail(NDWT_ERR_UNSUPPORTED, "a band of %lld elements: the order statistics count in 32 bits (fewer than 2^32 elements)", N);
    return NDWT_OK;
}

// select_passes(T) times: the histogram of one digit over the n scalars at y, then the pick; the state `st` and the histogram `ghist`
// (in the plan's select buffer, zero before the first pass) stay on the device in between.  Enqueued only.
extern "C++" template <typename T> static int select_passes_run(ndwt_plan* p, const T* y, long long n, SelectState* st, unsigned* ghist, int nk, const int64_t* k, hipStream_t s) {
    constexpr bool f64 = sizeof(T) == 8;
    void* const buf = p->select_buf.ptr;
    int rc = 0;
    const bool vec = select_vec((unsigned long long)(uintptr_t)y, n, (int)sizeof(T));
    const int nblocks = (int)select_grid(n, (int)p->comp, vec, p->num_cus, p->target_blocks);
    for (int pass = 0; pass < select_passes(f64); ++pass) {
        const int shift = select_digit_shift(f64, pass), bits = select_digit_bits(f64, pass), top = shift + bits;
        const unsigned long long himask = top >= select_key_bits(f64) ? 0ULL : ((~0ULL << top) & (f64 ? ~0ULL : 0xffffffffULL));
        const BandHistArgs<T> a = {y, n, st, ghist, himask, shift, bits, nk, nblocks};
        rc = launch_band_hist(a, (int)p->comp, vec, select_agg(p->variant_fwd), buf, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no histogram kernel for this data kind");
        if (rc != 0) return fail(NDWT_ERR_HIP, "histogram kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        BandPickArgs pa = {st, ghist, {0, 0, 0, 0}, nk, pass, shift};
        for (int i = 0; i < nk; ++i) pa.k[i] = (unsigned)k[i];
        rc = launch_band_pick(f64, pa, buf, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no pick kernel for this data kind");
        if (rc != 0) return fail(NDWT_ERR_HIP, "pick kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    return NDWT_OK;
}
// the passes over the whole band; one copy of the nk keys and one synchronisation of the stream end it
extern "C++" template <typename T> static int select_impl(ndwt_plan* p, const T* y, int nk, const int64_t* k, double* values, hipStream_t s) {
    int rc = p->select_buf.grow(kSelectBufBytes, "for the select state");
    if (rc) return rc;
    void* const buf = p->select_buf.ptr;
    SelectState* const st = (SelectState*)buf;
    HIP_TRY(hipMemsetAsync(buf, 0, kSelectBufBytes, s));
    rc = select_passes_run<T>(p, y, p->vol, st, (unsigned*)((char*)buf + sizeof(SelectState)), nk, k, s);
    if (rc) return rc;
    unsigned long long keys[kSelectMaxRanks] = {};
    HIP_TRY(hipMemcpyAsync(keys, st->prefix, sizeof(unsigned long long) * (size_t)nk, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < nk; ++i) {
        typename SelectKey<T>::type key = (typename SelectKey<T>::type)keys[i];
        T v;
        memcpy(&v, &key, sizeof v);
        values[i] = (double)v;
    }
    return NDWT_OK;
}

int ndwt_band_select(ndwt_plan* p, const void* y, int64_t band_pitch, int level, int64_t band, int nk, const int64_t* k, double* values, void* stream) {
    int rc = select_check(p, y, level, band, nk, k, values);
    if (rc) return rc;
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return select_impl(p, (const decltype(t)*)y + band * bs, nk, k, values, (hipStream_t)stream); });
}

// the gain of the last band of a level-1 transform of the plan's filtered axes (what ndwt_band_gains computes, from the same code)
static double last_band_gain(const ndwt_plan* p) {
    double g = 1.0;
    for (int a = 0; a < p->ndim; ++a) {
        double A[2], D[2];
        axis_gains(p->filt[a], p->dims[a], p->dilation == NDWT_DILATION_ATROUS, 1, A, D);
        g *= D[1];
    }
    return g;
}

int ndwt_estimate_sigma_coef(ndwt_plan* p, const void* y, int64_t band_pitch, int level, double* sigma, void* stream) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    if (!sigma) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (sigma)");
    const long long N = p->vol / p->comp;
    const int64_t k[2] = {(N - 1) / 2, N / 2};            // the middle, or the two middle order statistics of an even count
    const int nk = N % 2 ? 1 : 2;
    double v[2] = {0, 0};
    rc = ndwt_band_select(p, y, band_pitch, level, ndwt_num_bands(p->ndim, level) - 1, nk, k, v, stream);
    if (rc) return rc;
    if (p->sigma_gain == 0.0) p->sigma_gain = last_band_gain(p);
    const double m = nk == 2 ? 0.5 * (v[0] + v[1]) : v[0];
    // the median of |N(0, 1)|; complex data: of the Rayleigh distribution with unit parts, sqrt(2 ln 2)
    *sigma = m / (p->complexity == NDWT_REAL ? 0.6744897501960817 : 1.1774100225154747) / p->sigma_gain;
    return NDWT_OK;
}

int ndwt_estimate_sigma(ndwt_plan* p, const void* x, double* sigma, void* stream) {
    int rc = check_level(p, 1);
    if (rc) return rc;
    if (!x) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (x_dev)");
    if (!sigma) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (sigma)");
    rc = on_device(p, [&](auto t) {
        decltype(t)* coef = nullptr;
        long long bs = 0;
        return dec_scratch(p, (const decltype(t)*)x, 1, (hipStream_t)stream, &coef, &bs);
    });
    if (rc) return rc;
    return ndwt_estimate_sigma_coef(p, p->coef.ptr, ndwt_band_pitch(p), 1, sigma, stream);
}

// ---- the per-item forms: a statistic and a threshold row for every item of a batched plan (include/ndwt.h; the kernels:
// ndwt_device_items.h).  An item's part of a band is the item_vol() scalars at item * item_vol(); an unbatched plan is one item. ----
// select_check with the ranks inside ONE item, and the item's size against the 32-bit counters
static int select_items_check(const ndwt_plan* p, const void* y, int level, int64_t band, int nk, const int64_t* k, const double* values) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    if (!k) return fail(NDWT_ERR_INVALID_ARG, "null rank array (k)");
    if (!values) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (values)");
    const long long nb = ndwt_num_bands(p->ndim, level), N = p->item_vol() / p->comp;
    if (band < 0 || band >= nb) return fail(NDWT_ERR_INVALID_ARG, "band %lld outside 0..%lld of a level-%d coefficient array", (long long)band, nb - 1, level);
    if (nk < 1 || nk > kSelectMaxRanks) return fail(NDWT_ERR_INVALID_ARG, "nk = %d: 1..%d ranks per call", nk, kSelectMaxRanks);
    for (int i = 0; i < nk; ++i)
        if (k[i] < 0 || k[i] >= N) return fail(NDWT_ERR_INVALID_ARG, "k[%d] = %lld outside [0, %lld), the elements of one item of a band", i, (long long)k[i], N);
    if (!select_fits(N)) return fail(NDWT_ERR_UNSUPPORTED, "items of %lld elements: the order statistics count in 32 bits (fewer than 2^32 elements)", N);
    if (p->items() > 0x7fffffffLL) return fail(NDWT_ERR_UNSUPPORTED, "%lld items: the per-item order statistics serve fewer than 2^31", p->items());
    return NDWT_OK;
}

// By select_items_route: ItemSelect on `items` workgroups, or the passes of select_impl once per item.  Either way the keys of every
// item stay in the plan's select buffer behind the band-wide state and histogram; one copy and one synchronisation of the stream end it.
extern "C++" template <typename T> static int select_items_impl(ndwt_plan* p, const T* y, int nk, const int64_t* k, double* values, hipStream_t s) {
    const long long items = p->items(), n = p->item_vol();
    static_assert(sizeof(SelectState) >= sizeof(unsigned long long) * kSelectMaxRanks, "a state per item holds the keys of either route");
    int rc = p->select_buf.grow(kSelectBufBytes + (size_t)items * sizeof(SelectState), "for the select state");
    if (rc) return rc;
    char* const buf = (char*)p->select_buf.ptr;
    char* const per_item = buf + kSelectBufBytes;
    const bool one = select_items_route(n, items, p->num_cus, p->variant_inv) == kItemsOneLaunch;
    const size_t stride = one ? sizeof(unsigned long long) * kSelectMaxRanks : sizeof(SelectState);
    if (one) {
        ItemSelectArgs<T> a = {y, n, (unsigned long long*)per_item, {0, 0, 0, 0}, nk};
        for (int i = 0; i < nk; ++i) a.k[i] = (unsigned)k[i];
        rc = launch_item_select(a, (int)p->comp, select_vec((unsigned long long)(uintptr_t)y, n, (int)sizeof(T)), (int)items, buf, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no per-item select kernel for this data kind");
        if (rc != 0) return fail(NDWT_ERR_HIP, "per-item select kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    } else {
        HIP_TRY(hipMemsetAsync(buf, 0, kSelectBufBytes + (size_t)items * sizeof(SelectState), s));
        for (long long j = 0; j < items; ++j) {
            rc = select_passes_run<T>(p, y + j * n, n, (SelectState*)per_item + j, (unsigned*)(buf + sizeof(SelectState)), nk, k, s);
            if (rc) return rc;
        }
    }
    std::vector<unsigned long long> keys((size_t)items * stride / sizeof(unsigned long long));
    HIP_TRY(hipMemcpyAsync(keys.data(), per_item, (size_t)items * stride, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (long long j = 0; j < items; ++j)
        for (int i = 0; i < nk; ++i) {
            typename SelectKey<T>::type key = (typename SelectKey<T>::type)keys[(size_t)j * (stride / sizeof(unsigned long long)) + i];
            T v;
            memcpy(&v, &key, sizeof v);
            values[j * nk + i] = (double)v;
        }
    return NDWT_OK;
}

int ndwt_band_select_items(ndwt_plan* p, const void* y, int64_t band_pitch, int level, int64_t band, int nk, const int64_t* k, double* values, void* stream) {
    int rc = select_items_check(p, y, level, band, nk, k, values);
    if (rc) return rc;
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return select_items_impl(p, (const decltype(t)*)y + band * bs, nk, k, values, (hipStream_t)stream); });
}

int ndwt_estimate_sigma_coef_items(ndwt_plan* p, const void* y, int64_t band_pitch, int level, double* sigma, void* stream) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    if (!sigma) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (sigma)");
    const long long N = p->item_vol() / p->comp, items = p->items();
    const int64_t k[2] = {(N - 1) / 2, N / 2};            // the middle, or the two middle order statistics of an even count
    const int nk = N % 2 ? 1 : 2;
    std::vector<double> v((size_t)items * nk);
    rc = ndwt_band_select_items(p, y, band_pitch, level, ndwt_num_bands(p->ndim, level) - 1, nk, k, v.data(), stream);
    if (rc) return rc;
    if (p->sigma_gain == 0.0) p->sigma_gain = last_band_gain(p);
    for (long long j = 0; j < items; ++j) {
        const double m = nk == 2 ? 0.5 * (v[2 * j] + v[2 * j + 1]) : v[j];
        sigma[j] = m / (p->complexity == NDWT_REAL ? 0.6744897501960817 : 1.1774100225154747) / p->sigma_gain;
    }
    return NDWT_OK;
}

int ndwt_estimate_sigma_items(ndwt_plan* p, const void* x, double* sigma, void* stream) {
    int rc = check_level(p, 1);
    if (rc) return rc;
    if (!x) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (x_dev)");
    if (!sigma) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (sigma)");
    rc = on_device(p, [&](auto t) {
        decltype(t)* coef = nullptr;
        long long bs = 0;
        return dec_scratch(p, (const decltype(t)*)x, 1, (hipStream_t)stream, &coef, &bs);
    });
    if (rc) return rc;
    return ndwt_estimate_sigma_coef_items(p, p->coef.ptr, ndwt_band_pitch(p), 1, sigma, stream);
}

// bands_check for a table [items][nb]
static int items_table_check(const ndwt_plan* p, int level, const double* thr, int mode) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!thr) return fail(NDWT_ERR_INVALID_ARG, "null thresholds");
    const long long nb = ndwt_num_bands(p->ndim, level), items = p->items();
    for (long long j = 0; j < items; ++j)
        for (long long b = 0; b < nb; ++b)
            if (!(thr[j * nb + b] >= 0.0)) return fail(NDWT_ERR_INVALID_ARG, "threshold of item %lld, band %lld must be >= 0", j, b);
    if (mode != NDWT_SHRINK_SOFT && mode != NDWT_SHRINK_HARD) return fail(NDWT_ERR_INVALID_ARG, "mode must be NDWT_SHRINK_SOFT or NDWT_SHRINK_HARD");
    if (items > 0x7fffffffLL) return fail(NDWT_ERR_UNSUPPORTED, "%lld items: the per-item thresholds serve fewer than 2^31", items);
    return NDWT_OK;
}

// The table in the plan's scalar type (converted as shrink_run converts its threshold) on the device, by way of the plan's pinned buffer:
// the copy is enqueued on `s`, in order with the kernels of this and of earlier calls on that stream that read the device buffer.
extern "C++" template <typename T> static int items_table_upload(ndwt_plan* p, const double* thr, size_t count, hipStream_t s, const T** table) {
    const size_t bytes = count * sizeof(T);
    if (p->thr_copy_pending) {                            // the previous call's copy has left the pinned buffer before it is overwritten
        HIP_TRY(hipEventSynchronize(p->thr_event));
        p->thr_copy_pending = false;
    }
    if (bytes > p->thr_host_bytes) {
        if (p->thr_host) HIP_TRY(hipHostFree(p->thr_host));
        p->thr_host = nullptr;
        p->thr_host_bytes = 0;
        const size_t want = bytes < 4096 ? 4096 : bytes;
        const hipError_t e = hipHostMalloc(&p->thr_host, want, hipHostMallocDefault);
        if (e != hipSuccess) {
            p->thr_host = nullptr;
            return fail(NDWT_ERR_ALLOC, "hipHostMalloc(%zu bytes) for the threshold table failed: %s", want, hipGetErrorString(e));
        }
        p->thr_host_bytes = want;
    }
    if (!p->thr_event) HIP_TRY(hipEventCreateWithFlags(&p->thr_event, hipEventDisableTiming));
    const int rc = p->thr_dev.grow(p->thr_host_bytes, "for the threshold table");
    if (rc) return rc;
    T* const h = (T*)p->thr_host;
    for (size_t i = 0; i < count; ++i) h[i] = (T)thr[i];
    HIP_TRY(hipMemcpyAsync(p->thr_dev.ptr, h, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(p->thr_event, s));
    p->thr_copy_pending = true;
    *table = (const T*)p->thr_dev.ptr;
    return NDWT_OK;
}

// ShrinkItems on every (band, item) block in one launch; an all-zero table launches (and uploads) nothing.  Past 2^31 - 1 workgroups:
// one launch per band
extern "C++" template <typename T> static int shrink_items_impl(ndwt_plan* p, T* y, long long bs, int level, const double* thr, int mode, hipStream_t s) {
    const long long nb = ndwt_num_bands(p->ndim, level), items = p->items(), n = p->item_vol();
    bool any = false;
    for (long long i = 0; i < nb * items && !any; ++i) any = thr[i] != 0.0;
    if (!any) return NDWT_OK;
    const T* table = nullptr;
    int rc = items_table_upload<T>(p, thr, (size_t)(nb * items), s, &table);
    if (rc) return rc;
    const bool vec = aligned_vec4<T>(y) && bs % 4 == 0 && n % 4 == 0;
    const bool per_band = nb * items > 0x7fffffffLL;      // (items < 2^31: a band alone always fits)
    const long long chunks = shrink_items_chunks(n, (int)p->comp, vec, per_band ? 1 : nb, items, p->num_cus);
    ShrinkItemsArgs<T> a = {y, bs, n, table, items, (int)nb, 0, (int)nb, (int)chunks, mode};
    for (int b = 0; b < (per_band ? (int)nb : 1); ++b) {
        if (per_band) { a.band0 = b; a.nbands = 1; }
        rc = launch_shrink_items(a, (int)p->comp, vec, table, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no per-item shrink kernel for this data kind or grid");
        if (rc != 0) return fail(NDWT_ERR_HIP, "per-item shrink kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    return NDWT_OK;
}

int ndwt_shrink_bands_items(ndwt_plan* p, void* y, int64_t band_pitch, int level, const double* thresholds, int mode, void* stream) {
    int rc = items_table_check(p, level, thresholds, mode);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return shrink_items_impl(p, (decltype(t)*)y, bs, level, thresholds, mode, (hipStream_t)stream); });
}

// A batched 1-D plan: the whole depth in one launch with a threshold row per signal, under the conditions of ndwt_denoise_bands
// (denoise1_wanted / denoise1_levels, the pointers as denoise1_run asks) where the ROWTHR instance exists.  Else, and on every other plan
// kind: dec into the plan's pitched scratch, ShrinkItems, rec (no thresholding in the synthesis loads)
int ndwt_denoise_bands_items(ndwt_plan* p, const void* x, void* out, int level, const double* thresholds, int mode, void* stream) {
    int rc = items_table_check(p, level, thresholds, mode);
    if (rc) return rc;
    if (!x || !out) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    HIP_TRY(hipSetDevice(p->device));
    {
        const SelPlan sp = sel(p);
        const int n = denoise1_wanted(sp) ? denoise1_levels(sp, level) : 0;
        if (n && den1r_instantiated({sp.f64, sp.comp, sp.len[0], n})) {
            rc = with_scalar(p, [&](auto t) {
                typedef decltype(t) T;
                const T *xt = (const T*)x, *ot = (const T*)out;
                const size_t vol = (size_t)p->vol;
                if (!aligned_vec4<T>(x) || !aligned_vec4<T>(out) || !(xt + vol <= ot || ot + vol <= xt)) return -1;   // (before the table is uploaded)
                // the rows in the order of Den1CArgs::thr: the approximation, then the detail bands finest cascade level first
                const long long items = p->items(), nb = n + 1;
                std::vector<double> rows((size_t)items * 5, 0.0);
                for (long long j = 0; j < items; ++j) {
                    rows[5 * j] = thresholds[j * nb];
                    for (int l = 0; l < n; ++l) rows[5 * j + 1 + l] = thresholds[j * nb + 1 + (n - 1 - l)];
                }
                const T* table = nullptr;
                const int rc = items_table_upload<T>(p, rows.data(), rows.size(), (hipStream_t)stream, &table);
                if (rc) return rc;
                return denoise1_run<T>(p, p->filt[0].len, n, xt, (T*)out, nullptr, mode, (hipStream_t)stream, table);
            });
            if (rc != -1) return rc;                      // -1: not this data -- the general route, silently
        }
    }
    return on_device(p, [&](auto t) {
        typedef decltype(t) T;
        T* coef = nullptr;
        long long bs = 0;
        int rc = dec_scratch<T>(p, (const T*)x, level, (hipStream_t)stream, &coef, &bs);
        if (rc == NDWT_OK) rc = shrink_items_impl<T>(p, coef, bs, level, thresholds, mode, (hipStream_t)stream);
        if (rc == NDWT_OK) rc = rec_impl<T>(p, coef, bs, (T*)out, level, kNoShrink, (hipStream_t)stream);
        return rc;
    });
}

// ---- the band norms: l1, energy, max and non-zeros of every (band, item) block in one read (include/ndwt.h; the kernels:
// ndwt_device_norms.h) ----
// select_items_check without the band and the ranks
static int norms_check(const ndwt_plan* p, const void* y, int level, const double* norms, const char* norms_name) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    if (!norms) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (%s)", norms_name);
    if (p->items() > 0x7fffffffLL) return fail(NDWT_ERR_UNSUPPORTED, "%lld items: the band norms serve fewer than 2^31", p->items());
    return NDWT_OK;
}

// BandNorms on every (band, item) block of `items` items of n scalars in one launch, by norms_chunks; with more than one chunk the
// partials go to the plan's buffer and NormsFinish combines them.  out_dev: [items][nb][4] doubles, or null: the results' place in the
// plan's buffer (returned in *res).  Past 2^31 - 1 workgroups: one launch per band.  Enqueued only.
extern "C++" template <typename T> static int norms_run(ndwt_plan* p, const T* y, long long bs, int level, long long items, long long n, double* out_dev, double** res,
                                                        hipStream_t s) {
    const long long nb = ndwt_num_bands(p->ndim, level);
    const bool vec = aligned_vec4<T>(y) && bs % 4 == 0 && n % 4 == 0;
    const bool per_band = norms_per_band(nb, items);
    const long long chunks = norms_chunks(n, (int)p->comp, vec, per_band ? 1 : nb, items, p->num_cus, p->target_blocks);
    const size_t res_bytes = (size_t)(nb * items) * 4 * sizeof(double);
    int rc = p->norms_buf.grow(res_bytes * (chunks > 1 ? 1 + (size_t)chunks : 1), "for the band norms");
    if (rc) return rc;
    double* const results = out_dev ? out_dev : (double*)p->norms_buf.ptr;
    double* const partials = (double*)((char*)p->norms_buf.ptr + res_bytes);
    BandNormsArgs<T> a = {y, bs, n, chunks > 1 ? partials : results, items, (int)nb, 0, (int)nb, (int)chunks};
    NormsFinishArgs f = {partials, results, items, (int)nb, 0, (int)nb, (int)chunks};
    for (int b = 0; b < (per_band ? (int)nb : 1); ++b) {
        if (per_band) { a.band0 = f.band0 = b; a.nbands = f.nbands = 1; }
        rc = launch_band_norms(a, (int)p->comp, vec, p->norms_buf.ptr, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no band-norms kernel for this data kind or grid");
        if (rc != 0) return fail(NDWT_ERR_HIP, "band-norms kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        if (chunks == 1) continue;
        rc = launch_norms_finish(f, p->norms_buf.ptr, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: a grid the band-norms combine cannot express");
        if (rc != 0) return fail(NDWT_ERR_HIP, "band-norms combine launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    if (res) *res = results;
    return NDWT_OK;
}

// the host forms: the launches, then one copy of the results and one synchronisation of the stream
static int norms_host(ndwt_plan* p, const void* y, int64_t band_pitch, int level, bool per_item, double* norms, void* stream) {
    int rc = norms_check(p, y, level, norms, "norms");
    if (rc) return rc;
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    const long long items = per_item ? p->items() : 1, n = per_item ? p->item_vol() : p->vol;
    return on_device(p, [&](auto t) {
        double* res = nullptr;
        const int rc = norms_run(p, (const decltype(t)*)y, bs, level, items, n, nullptr, &res, (hipStream_t)stream);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(norms, res, (size_t)(ndwt_num_bands(p->ndim, level) * items) * 4 * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return (int)NDWT_OK;
    });
}

int ndwt_band_norms(ndwt_plan* p, const void* y, int64_t band_pitch, int level, double* norms, void* stream) {
    return norms_host(p, y, band_pitch, level, false, norms, stream);
}

int ndwt_band_norms_items(ndwt_plan* p, const void* y, int64_t band_pitch, int level, double* norms, void* stream) {
    return norms_host(p, y, band_pitch, level, true, norms, stream);
}

int ndwt_band_norms_dev(ndwt_plan* p, const void* y, int64_t band_pitch, int level, int per_item, double* norms_dev, void* stream) {
    int rc = norms_check(p, y, level, norms_dev, "norms_dev");
    if (rc) return rc;
    if ((uintptr_t)norms_dev % sizeof(double) != 0) return fail(NDWT_ERR_INVALID_ARG, "norms_dev must be 8-byte aligned");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    const long long items = per_item ? p->items() : 1, n = per_item ? p->item_vol() : p->vol;
    return on_device(p, [&](auto t) { return norms_run(p, (const decltype(t)*)y, bs, level, items, n, norms_dev, nullptr, (hipStream_t)stream); });
}

// ---- the SURE statistics: count, energy and reciprocal sum of every (band, item) block at up to NDWT_RISK_MAX_CAND thresholds in one
// read (include/ndwt.h; the kernels: ndwt_device_risk.h) ----
// norms_check, and the candidate table [items][nb][nc]: every entry >= 0 (+inf included), but a row may begin with a negative one
static int risk_check(const ndwt_plan* p, const void* y, int level, bool per_item, int nc, const double* cand, const double* risk) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    if (!cand) return fail(NDWT_ERR_INVALID_ARG, "null candidate thresholds (cand)");
    if (!risk) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (risk)");
    if (nc < 1 || nc > NDWT_RISK_MAX_CAND) return fail(NDWT_ERR_INVALID_ARG, "nc = %d outside 1..%d candidates", nc, NDWT_RISK_MAX_CAND);
    if (p->items() > 0x7fffffffLL) return fail(NDWT_ERR_UNSUPPORTED, "%lld items: the band risk serves fewer than 2^31", p->items());
    const long long nb = ndwt_num_bands(p->ndim, level), items = per_item ? p->items() : 1;
    for (long long j = 0; j < items; ++j)
        for (long long b = 0; b < nb; ++b)
            for (int i = 0; i < nc; ++i) {
                const double t = cand[(j * nb + b) * nc + i];
                if (t >= 0.0 || (i == 0 && t < 0.0)) continue;
                if (per_item) return fail(NDWT_ERR_INVALID_ARG, "cand of item %lld, band %lld, position %d must be >= 0 (a negative first entry skips the block)", j, b, i);
                return fail(NDWT_ERR_INVALID_ARG, "cand of band %lld, position %d must be >= 0 (a negative first entry skips the block)", b, i);
            }
    return NDWT_OK;
}

// BandRisk on every (band, item) block of `items` items of n scalars in one launch, on the grid of norms_run; with more than one chunk
// the partials go behind the results in the plan's buffer and RiskFinish combines them.  The results' place is returned in *res.
// Enqueued only (but for the wait of items_table_upload).
extern "C++" template <typename T> static int risk_run(ndwt_plan* p, const T* y, long long bs, int level, long long items, long long n, int nc, const double* cand,
                                                       double** res, hipStream_t s) {
    const long long nb = ndwt_num_bands(p->ndim, level);
    const bool vec = aligned_vec4<T>(y) && bs % 4 == 0 && n % 4 == 0;
    const bool per_band = norms_per_band(nb, items);
    const long long chunks = norms_chunks(n, (int)p->comp, vec, per_band ? 1 : nb, items, p->num_cus, p->target_blocks);
    if (risk_thread_elements(n, (int)p->comp, vec, chunks) > 0xffffffffLL)
        return fail(NDWT_ERR_UNSUPPORTED, "a block of %lld elements on %lld workgroups: a thread of the band risk counts fewer than 2^32", n / p->comp, chunks);
    const T* table = nullptr;
    int rc = items_table_upload<T>(p, cand, (size_t)(nb * items) * nc, s, &table);
    if (rc) return rc;
    const size_t res_bytes = (size_t)(nb * items) * nc * 3 * sizeof(double);
    rc = p->norms_buf.grow(res_bytes * (chunks > 1 ? 1 + (size_t)chunks : 1), "for the band risk");
    if (rc) return rc;
    double* const results = (double*)p->norms_buf.ptr;
    double* const partials = (double*)((char*)p->norms_buf.ptr + res_bytes);
    BandRiskArgs<T> a = {y, bs, n, table, chunks > 1 ? partials : results, items, (int)nb, 0, (int)nb, (int)chunks, nc};
    RiskFinishArgs f = {partials, results, items, (int)nb, 0, (int)nb, (int)chunks, nc};
    for (int b = 0; b < (per_band ? (int)nb : 1); ++b) {
        if (per_band) { a.band0 = f.band0 = b; a.nbands = f.nbands = 1; }
        rc = launch_band_risk(a, (int)p->comp, vec, p->norms_buf.ptr, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no band-risk kernel for this data kind or grid");
        if (rc != 0) return fail(NDWT_ERR_HIP, "band-risk kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        if (chunks == 1) continue;
        rc = launch_risk_finish(f, p->norms_buf.ptr, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: a grid the band-risk combine cannot express");
        if (rc != 0) return fail(NDWT_ERR_HIP, "band-risk combine launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    *res = results;
    return NDWT_OK;
}

// the launches, then one copy of the results and one synchronisation of the stream
static int risk_host(ndwt_plan* p, const void* y, int64_t band_pitch, int level, bool per_item, int nc, const double* cand, double* risk, void* stream) {
    int rc = risk_check(p, y, level, per_item, nc, cand, risk);
    if (rc) return rc;
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    const long long items = per_item ? p->items() : 1, n = per_item ? p->item_vol() : p->vol;
    return on_device(p, [&](auto t) {
        double* res = nullptr;
        const int rc = risk_run(p, (const decltype(t)*)y, bs, level, items, n, nc, cand, &res, (hipStream_t)stream);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(risk, res, (size_t)(ndwt_num_bands(p->ndim, level) * items) * nc * 3 * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return (int)NDWT_OK;
    });
}

int ndwt_band_risk(ndwt_plan* p, const void* y, int64_t band_pitch, int level, int nc, const double* cand, double* risk, void* stream) {
    return risk_host(p, y, band_pitch, level, false, nc, cand, risk, stream);
}

int ndwt_band_risk_items(ndwt_plan* p, const void* y, int64_t band_pitch, int level, int nc, const double* cand, double* risk, void* stream) {
    return risk_host(p, y, band_pitch, level, true, nc, cand, risk, stream);
}

int ndwt_sure_from_risk(int comp, double n, double s, int nc, const double* cand, const double* risk, double* sure) {
    if (comp != 1 && comp != 2) return fail(NDWT_ERR_INVALID_ARG, "comp must be 1 (real) or 2 (complex)");
    if (!(n >= 0.0) || std::isinf(n)) return fail(NDWT_ERR_INVALID_ARG, "n must be finite and >= 0");
    if (!(s >= 0.0) || std::isinf(s)) return fail(NDWT_ERR_INVALID_ARG, "s must be finite and >= 0");
    if (nc < 1) return fail(NDWT_ERR_INVALID_ARG, "nc must be >= 1");
    if (!cand) return fail(NDWT_ERR_INVALID_ARG, "null candidate thresholds (cand)");
    if (!risk) return fail(NDWT_ERR_INVALID_ARG, "null statistics (risk)");
    if (!sure) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (sure)");
    const double d = comp, s2 = s * s;
    for (int i = 0; i < nc; ++i) {
        const double t = cand[i], C = risk[3 * i + NDWT_RISK_COUNT], E = risk[3 * i + NDWT_RISK_ENERGY], I = risk[3 * i + NDWT_RISK_INVSUM];
        // (t = +inf leaves nothing above it: n - C and I are 0, and their terms are dropped, not inf * 0)
        const double above = n - C == 0.0 ? 0.0 : t * t * (n - C), curl = comp == 1 || I == 0.0 ? 0.0 : (d - 1.0) * t * I;
        sure[i] = n * d * s2 + E + above - 2.0 * s2 * (d * C + curl);
    }
    return NDWT_OK;
}

// the gains of the bands of a transform of the plan's filtered axes (what ndwt_band_gains computes, from the same code)
static void plan_band_gains(const ndwt_plan* p, int level, double* gains) {
    std::vector<double> A[NDWT_MAX_DIMS], D[NDWT_MAX_DIMS];
    for (int a = 0; a < p->ndim; ++a) {
        A[a].resize((size_t)level + 1);
        D[a].resize((size_t)level + 1);
        axis_gains(p->filt[a], p->dims[a], p->dilation == NDWT_DILATION_ATROUS, level, A[a].data(), D[a].data());
    }
    const int nb = 1 << p->ndim;
    const long long bands = ndwt_num_bands(p->ndim, level);
    for (long long b = 0; b < bands; ++b) {
        const int lev = b == 0 ? level : level - (int)((b - 1) / (nb - 1));
        const int bits = b == 0 ? 0 : 1 + (int)((b - 1) % (nb - 1));
        double g = 1.0;
        for (int a = 0; a < p->ndim; ++a) g *= ((bits >> a) & 1) ? D[a][(size_t)lev] : A[a][(size_t)lev];
        gains[b] = g;
    }
}

// The search of ndwt_sure_thresholds(_items) (include/ndwt.h): every round is ONE ndwt_band_risk(_items) call over all blocks, 8
// candidates a block on its own interval; band 0 and the blocks with nothing to search (s = 0, one element) are skipped rows.
static int sure_search(ndwt_plan* p, const void* y, int64_t band_pitch, int level, bool per_item, const double* sigma, int rounds, double* thresholds, double* sure,
                       void* stream) {
    int rc = check_level(p, level);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    if (!sigma) return fail(NDWT_ERR_INVALID_ARG, "null sigma");
    if (!thresholds) return fail(NDWT_ERR_INVALID_ARG, "null output pointer (thresholds)");
    if (rounds < 0 || rounds > 8) return fail(NDWT_ERR_INVALID_ARG, "rounds = %d outside 1..8 (0: the default, 3)", rounds);
    if (p->items() > 0x7fffffffLL) return fail(NDWT_ERR_UNSUPPORTED, "%lld items: the band risk serves fewer than 2^31", p->items());
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);               // (before anything is written: a refused call leaves its outputs alone)
    if (rc) return rc;
    const long long nb = ndwt_num_bands(p->ndim, level), items = per_item ? p->items() : 1, blocks = nb * items;
    for (long long j = 0; j < items; ++j)
        if (!(sigma[j] >= 0.0) || std::isinf(sigma[j])) {
            if (per_item) return fail(NDWT_ERR_INVALID_ARG, "sigma of item %lld must be finite and >= 0", j);
            return fail(NDWT_ERR_INVALID_ARG, "sigma must be finite and >= 0");
        }
    if (rounds == 0) rounds = 3;
    constexpr int NC = NDWT_RISK_MAX_CAND;
    const bool f32 = p->dtype == NDWT_F32;
    const double d = (double)p->comp;
    double N = 1.0;                                       // elements of ONE item's filtered axes
    for (int a = 0; a < p->ndim; ++a) N *= (double)p->dims[a];
    const double n = (double)((per_item ? p->item_vol() : p->vol) / p->comp);   // elements of a block
    std::vector<double> gains((size_t)nb), s((size_t)blocks), tmax((size_t)blocks), lo((size_t)blocks, 0.0), hi((size_t)blocks), best_r((size_t)blocks);
    std::vector<double> cand((size_t)blocks * NC), risk((size_t)blocks * NC * 3);
    plan_band_gains(p, level, gains.data());
    for (long long k = 0; k < blocks; ++k) {
        s[k] = sigma[k / nb] * gains[k % nb];
        tmax[k] = hi[k] = k % nb == 0 ? 0.0 : s[k] * std::sqrt(2.0 * std::log(N));
        thresholds[k] = 0.0;
        best_r[k] = k % nb == 0 ? 0.0 : n * d * s[k] * s[k];
    }
    for (int r = 0; r < rounds; ++r) {
        bool any = false;
        for (long long k = 0; k < blocks; ++k) {
            double* const c = &cand[(size_t)k * NC];
            if (!(tmax[k] > 0.0)) {                       // band 0, s = 0, one element: a skipped row
                c[0] = -1.0;
                for (int i = 1; i < NC; ++i) c[i] = 0.0;
                continue;
            }
            any = true;
            for (int i = 0; i < NC; ++i) {                // rounded as the shrink rounds its threshold: the statistics are those of what it applies
                const double t = lo[k] + (hi[k] - lo[k]) * (double)(i + 1) / 8.0;
                c[i] = f32 ? (double)(float)t : t;
            }
        }
        if (!any) break;
        rc = risk_host(p, y, band_pitch, level, per_item, NC, cand.data(), risk.data(), stream);
        if (rc) return rc;
        for (long long k = 0; k < blocks; ++k) {
            if (!(tmax[k] > 0.0)) continue;
            double v[NC];
            (void)ndwt_sure_from_risk((int)p->comp, n, s[k], NC, &cand[(size_t)k * NC], &risk[(size_t)k * NC * 3], v);
            int at = 0;
            for (int i = 1; i < NC; ++i)
                if (v[i] < v[at] || (v[at] != v[at] && v[i] == v[i])) at = i;   // the first of the smallest (a NaN is never smaller)
            if (v[at] < best_r[k]) { best_r[k] = v[at]; thresholds[k] = cand[(size_t)k * NC + at]; }
            const double step = (hi[k] - lo[k]) / 8.0;
            lo[k] = std::max(thresholds[k] - step, 0.0);
            hi[k] = std::min(thresholds[k] + step, tmax[k]);
        }
    }
    if (sure)
        for (long long k = 0; k < blocks; ++k) sure[k] = best_r[k];
    return NDWT_OK;
}

int ndwt_sure_thresholds(ndwt_plan* p, const void* y, int64_t band_pitch, int level, double sigma, int rounds, double* thresholds, double* sure, void* stream) {
    return sure_search(p, y, band_pitch, level, false, &sigma, rounds, thresholds, sure, stream);
}

int ndwt_sure_thresholds_items(ndwt_plan* p, const void* y, int64_t band_pitch, int level, const double* sigma, int rounds, double* thresholds, double* sure,
                               void* stream) {
    return sure_search(p, y, band_pitch, level, true, sigma, rounds, thresholds, sure, stream);
}

// ---- joint shrinkage across the items of a plan and the norms of the groups (include/ndwt.h; the kernels: ndwt_device_joint.h) ----
// JointShrink on every band in one launch, by joint_chunks -- or JointTile, by joint_tile_strips, where joint_route names it; the
// thresholds [nb] go up as a table of one row.  An all-zero array launches (and uploads) nothing.
extern "C++" template <typename T> static int joint_shrink_impl(ndwt_plan* p, T* y, long long bs, int level, const double* thr, int mode, hipStream_t s) {
    const long long nb = ndwt_num_bands(p->ndim, level), items = p->items(), n = p->item_vol();
    bool any = false;
    for (long long b = 0; b < nb && !any; ++b) any = thr[b] != 0.0;
    if (!any) return NDWT_OK;
    const T* table = nullptr;
    int rc = items_table_upload<T>(p, thr, (size_t)nb, s, &table);
    if (rc) return rc;
    const bool vec = aligned_vec4<T>(y) && bs % 4 == 0 && n % 4 == 0;
    const bool tile = joint_route(n, (int)p->comp, vec, nb, items, p->num_cus, p->variant_inv) == kJointTile;
    const long long chunks = tile ? joint_tile_strips(n, (int)p->comp, vec) : joint_chunks(n, (int)p->comp, vec, nb, items, p->num_cus, p->target_blocks);
    const JointShrinkArgs<T> a = {y, bs, n, table, items, (int)nb, (int)chunks, mode};
    rc = tile ? launch_joint_tile(a, (int)p->comp, vec, table, s) : launch_joint_shrink(a, (int)p->comp, vec, items <= kJointReg, table, s);
    if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no joint shrink kernel for this data kind or grid");
    if (rc != 0) return fail(NDWT_ERR_HIP, "joint shrink kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    return NDWT_OK;
}

int ndwt_shrink_joint(ndwt_plan* p, void* y, int64_t band_pitch, int level, const double* thresholds, int mode, void* stream) {
    int rc = bands_check(p, level, thresholds, mode);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return joint_shrink_impl(p, (decltype(t)*)y, bs, level, thresholds, mode, (hipStream_t)stream); });
}

// the general route only: dec into the plan's pitched scratch, JointShrink, rec (no thresholding in the synthesis loads)
int ndwt_denoise_joint(ndwt_plan* p, const void* x, void* out, int level, const double* thresholds, int mode, void* stream) {
    int rc = bands_check(p, level, thresholds, mode);
    if (rc) return rc;
    if (!x || !out) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (x_dev or out_dev)");
    return on_device(p, [&](auto t) {
        typedef decltype(t) T;
        T* coef = nullptr;
        long long bs = 0;
        int rc = dec_scratch<T>(p, (const T*)x, level, (hipStream_t)stream, &coef, &bs);
        if (rc == NDWT_OK) rc = joint_shrink_impl<T>(p, coef, bs, level, thresholds, mode, (hipStream_t)stream);
        if (rc == NDWT_OK) rc = rec_impl<T>(p, coef, bs, (T*)out, level, kNoShrink, (hipStream_t)stream);
        return rc;
    });
}

// GroupNorms on every band in one launch, by joint_chunks -- or GroupNormsTile, by joint_tile_strips, where joint_route names it; with
// more than one chunk (strip) the partials go to the plan's buffer and NormsFinish (one item) combines them.  out_dev: [nb][4] doubles, or null: the results' place in the plan's
// buffer (returned in *res).  Enqueued only.
extern "C++" template <typename T> static int group_norms_run(ndwt_plan* p, const T* y, long long bs, int level, double* out_dev, double** res, hipStream_t s) {
    const long long nb = ndwt_num_bands(p->ndim, level), items = p->items(), n = p->item_vol();
    const bool vec = aligned_vec4<T>(y) && bs % 4 == 0 && n % 4 == 0;
    const bool tile = joint_route(n, (int)p->comp, vec, nb, items, p->num_cus, p->variant_inv) == kJointTile;
    const long long chunks = tile ? joint_tile_strips(n, (int)p->comp, vec) : joint_chunks(n, (int)p->comp, vec, nb, items, p->num_cus, p->target_blocks);
    const size_t res_bytes = (size_t)nb * 4 * sizeof(double);
    int rc = p->norms_buf.grow(res_bytes * (chunks > 1 ? 1 + (size_t)chunks : 1), "for the group norms");
    if (rc) return rc;
    double* const results = out_dev ? out_dev : (double*)p->norms_buf.ptr;
    double* const partials = (double*)((char*)p->norms_buf.ptr + res_bytes);
    const GroupNormsArgs<T> a = {y, bs, n, chunks > 1 ? partials : results, items, (int)nb, (int)chunks};
    rc = tile ? launch_group_norms_tile(a, (int)p->comp, vec, p->norms_buf.ptr, s) : launch_group_norms(a, (int)p->comp, vec, p->norms_buf.ptr, s);
    if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no group-norms kernel for this data kind or grid");
    if (rc != 0) return fail(NDWT_ERR_HIP, "group-norms kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (chunks > 1) {
        const NormsFinishArgs f = {partials, results, 1, (int)nb, 0, (int)nb, (int)chunks};
        rc = launch_norms_finish(f, p->norms_buf.ptr, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: a grid the group-norms combine cannot express");
        if (rc != 0) return fail(NDWT_ERR_HIP, "group-norms combine launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    if (res) *res = results;
    return NDWT_OK;
}

int ndwt_group_norms(ndwt_plan* p, const void* y, int64_t band_pitch, int level, double* norms, void* stream) {
    int rc = norms_check(p, y, level, norms, "norms");
    if (rc) return rc;
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) {
        double* res = nullptr;
        const int rc = group_norms_run(p, (const decltype(t)*)y, bs, level, nullptr, &res, (hipStream_t)stream);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(norms, res, (size_t)ndwt_num_bands(p->ndim, level) * 4 * sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return (int)NDWT_OK;
    });
}

int ndwt_group_norms_dev(ndwt_plan* p, const void* y, int64_t band_pitch, int level, double* norms_dev, void* stream) {
    int rc = norms_check(p, y, level, norms_dev, "norms_dev");
    if (rc) return rc;
    if ((uintptr_t)norms_dev % sizeof(double) != 0) return fail(NDWT_ERR_INVALID_ARG, "norms_dev must be 8-byte aligned");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) { return group_norms_run(p, (const decltype(t)*)y, bs, level, norms_dev, nullptr, (hipStream_t)stream); });
}

// ---- neighbourhood shrinkage: the energy of a window inside a coefficient's own band decides it (include/ndwt.h; the kernel:
// ndwt_device_neigh.h) ----
// what both entry points check, before any device call
static int neigh_check(const ndwt_plan* p, int level, int radius, const double* thr, int mode) {
    int rc = bands_check(p, level, thr, mode);
    if (rc) return rc;
    if (radius < 1 || radius > 3) return fail(NDWT_ERR_INVALID_ARG, "radius %d outside 1..3", radius);
    if (p->inner > 1)
        return fail(NDWT_ERR_UNSUPPORTED, "neighbourhood shrinkage does not serve interleaved plans: the neighbours of an element lie inner = %lld elements apart", p->inner);
    if (p->ndim > 3) return fail(NDWT_ERR_UNSUPPORTED, "neighbourhood shrinkage serves 1 to 3 filtered axes, this plan has %d", p->ndim);
    for (int k = 0; k < p->ndim; ++k)
        if (p->dims[k] < 2 * radius + 1)
            return fail(NDWT_ERR_UNSUPPORTED, "filtered axis %d has %lld elements, fewer than the window of 2 * radius + 1 = %d: the window would count an element twice", k,
                        p->dims[k], 2 * radius + 1);
    for (int k = 0; k < p->ndim; ++k)
        if (p->dims[k] > 0x7fffffffLL || p->dims[0] * (p->ndim == 3 ? p->dims[1] : 1) * p->comp > 0x7fffffffLL)
            return fail(NDWT_ERR_UNSUPPORTED, "neighbourhood shrinkage serves items whose lines (planes, with 3 filtered axes) stay below 2^31 scalars");
    return NDWT_OK;
}

// NeighShrink from y into out, both at the pitch bs.  The squared thresholds go up in double as a table of one row (items_table_upload);
// a band whose threshold is 0 has -1 there: copied.  out apart from y: every (band, item) block in ONE launch, by neigh_geometry; an
// all-zero array uploads nothing and launches nothing, the bands are copied.  out == y - bs: band b is written where band b - 1 was
// read, so the bands run in ascending order, one launch each in stream order, a zero-threshold band as one copy.
extern "C++" template <typename T> static int neigh_shrink_impl(ndwt_plan* p, const T* y, T* out, long long bs, int level, int radius, const double* thr, int mode,
                                                                hipStream_t s) {
    const long long nb = ndwt_num_bands(p->ndim, level), items = p->items(), n = p->item_vol();
    const uintptr_t yb = (uintptr_t)y, ob = (uintptr_t)out, span = (uintptr_t)((nb - 1) * bs + p->vol) * sizeof(T);
    const bool shifted = ob + (uintptr_t)bs * sizeof(T) == yb;
    if (!shifted && !(yb + span <= ob || ob + span <= yb))
        return fail(NDWT_ERR_INVALID_ARG, "out_dev overlaps y_dev (the one form allowed: out_dev == y_dev - band_pitch, the output one band slot down)");
    std::vector<double> tt((size_t)nb);
    bool any = false;
    for (long long b = 0; b < nb; ++b) {
        const T t = (T)thr[b];
        tt[b] = thr[b] == 0.0 ? -1.0 : (double)t * (double)t;
        any = any || thr[b] != 0.0;
    }
    const auto copy_band = [&](long long b) { return hipMemcpyAsync(out + b * bs, y + b * bs, (size_t)p->vol * sizeof(T), hipMemcpyDeviceToDevice, s); };
    if (!any) {
        for (long long b = 0; b < nb; ++b) HIP_TRY(copy_band(b));
        return NDWT_OK;
    }
    const double* table = nullptr;
    int rc = items_table_upload<double>(p, tt.data(), (size_t)nb, s, &table);
    if (rc) return rc;
    const int nd = p->ndim;
    const NeighGeom g = neigh_geometry(nd, p->dims[0], nd >= 2 ? p->dims[1] : 1, nd == 3 ? p->dims[2] : 1, (int)(sizeof(T) * p->comp), radius,
                                       (shifted ? 1 : nb) * items, p->num_cus, p->target_blocks);
    NeighArgs<T> a = {y, out, bs, n, table, items, (int)p->dims[0], nd >= 2 ? (int)p->dims[1] : 1, nd == 3 ? (int)p->dims[2] : 1, 0, (int)nb,
                      (int)g.ntx, (int)g.nty, (int)g.chunk, (int)g.nchunks, mode};
    for (long long b = 0; b < (shifted ? nb : 1); ++b) {
        if (shifted) {
            if (thr[b] == 0.0) { HIP_TRY(copy_band(b)); continue; }
            a.band0 = (int)b;
            a.nbands = 1;
        }
        rc = launch_neigh_shrink(a, (int)p->comp, nd, radius, table, s);
        if (rc < 0) return fail(NDWT_ERR_UNSUPPORTED, "internal: no neighbourhood shrink kernel for this data kind or grid");
        if (rc != 0) return fail(NDWT_ERR_HIP, "neighbourhood shrink kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    return NDWT_OK;
}

int ndwt_shrink_neigh(ndwt_plan* p, const void* y, void* out, int64_t band_pitch, int level, int radius, const double* thresholds, int mode, void* stream) {
    int rc = neigh_check(p, level, radius, thresholds, mode);
    if (rc) return rc;
    if (!y) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (y_dev)");
    if (!out) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (out_dev)");
    long long bs = 0;
    rc = pitch_scalars(p, band_pitch, &bs);
    if (rc) return rc;
    return on_device(p, [&](auto t) {
        return neigh_shrink_impl(p, (const decltype(t)*)y, (decltype(t)*)out, bs, level, radius, thresholds, mode, (hipStream_t)stream);
    });
}

// dec into slots 1 .. nb of the plan's pitched scratch (grown by one slot, once), the shrink one slot down, rec from slot 0
int ndwt_denoise_neigh(ndwt_plan* p, const void* x, void* out, int level, int radius, const double* thresholds, int mode, void* stream) {
    int rc = neigh_check(p, level, radius, thresholds, mode);
    if (rc) return rc;
    if (!x || !out) return fail(NDWT_ERR_INVALID_ARG, "null data pointer (x_dev or out_dev)");
    return on_device(p, [&](auto t) {
        typedef decltype(t) T;
        const long long bs = (long long)ndwt_band_pitch(p) * p->comp;
        int rc = p->coef.grow((size_t)bs * p->esize * (size_t)(ndwt_num_bands(p->ndim, level) + 1), "for the coefficient scratch");
        if (rc) return rc;
        T* const slot0 = (T*)p->coef.ptr;
        rc = dec_impl<T>(p, (const T*)x, slot0 + bs, bs, level, (hipStream_t)stream);
        if (rc == NDWT_OK) rc = neigh_shrink_impl<T>(p, slot0 + bs, slot0, bs, level, radius, thresholds, mode, (hipStream_t)stream);
        if (rc == NDWT_OK) rc = rec_impl<T>(p, slot0, bs, (T*)out, level, kNoShrink, (hipStream_t)stream);
        return rc;
    });
}

int ndwt_denoise_host(ndwt_plan* p, const void* x, void* out, int level, double threshold, int mode) {
    int rc = refuse_batched(p, "a host-pointer transform");
    if (rc) return rc;
    rc = shrink_check(p, level, threshold, mode);
    if (rc) return rc;
    if (!x || !out) return fail(NDWT_ERR_INVALID_ARG, "null data pointer");
    HIP_TRY(hipSetDevice(p->device));
    const size_t bx = (size_t)p->vol * p->esize;
    rc = ensure_stage(p, 0, 2 * bx);                      // the signal and the result, side by side (kept across calls)
    if (rc) return rc;
    void *dx = p->stage[0].ptr, *dout = (char*)dx + bx;
    hipError_t e = hipMemcpy(dx, x, bx, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = ndwt_denoise(p, dx, dout, level, threshold, mode, nullptr);
        if (rc == NDWT_OK) e = hipMemcpy(out, dout, bx, hipMemcpyDeviceToHost);
    }
    if (rc) return rc;
    if (e != hipSuccess) return fail(NDWT_ERR_HIP, "staging copy failed: %s", hipGetErrorString(e));
    return NDWT_OK;
}

// Split complex (separate real / imaginary arrays: mxGetPr / mxGetPi of nd_dwt_mex.c:55-58).  The filters are
// real, so the complex transform is the real transform of each part: a REAL plan is run once per part.
// one(in, out): the real transform of one part
extern "C++" template <class F> static int split_run(const ndwt_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im, F&& one) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    if (p->comp != 1) return fail(NDWT_ERR_INVALID_ARG, "split-complex entry points take a plan created with NDWT_REAL");
    if ((in_im == nullptr) != (out_im == nullptr)) return fail(NDWT_ERR_INVALID_ARG, "imaginary input and output must both be given or both be NULL");
    int rc = one(in_re, out_re);
    if (rc == NDWT_OK && in_im) rc = one(in_im, out_im);
    return rc;
}

int ndwt_dec_split(ndwt_plan* p, const void* x_re, const void* x_im, void* y_re, void* y_im, int level, void* stream) {
    return split_run(p, x_re, x_im, y_re, y_im, [&](const void* x, void* y) { return ndwt_dec(p, x, y, level, stream); });
}
int ndwt_rec_split(ndwt_plan* p, const void* y_re, const void* y_im, void* x_re, void* x_im, int level, void* stream) {
    return split_run(p, y_re, y_im, x_re, x_im, [&](const void* y, void* x) { return ndwt_rec(p, y, x, level, stream); });
}
int ndwt_dec_split_host(ndwt_plan* p, const void* x_re, const void* x_im, void* y_re, void* y_im, int level) {
    return split_run(p, x_re, x_im, y_re, y_im, [&](const void* x, void* y) { return host_roundtrip(p, false, x, y, level); });
}
int ndwt_rec_split_host(ndwt_plan* p, const void* y_re, const void* y_im, void* x_re, void* x_im, int level) {
    return split_run(p, y_re, y_im, x_re, x_im, [&](const void* y, void* x) { return host_roundtrip(p, true, y, x, level); });
}

int ndwt_plan_slab_fast(const ndwt_plan* p) {
    return p && slab_fused3(sel(p), 1, -1, slab_mode(p)) ? 1 : 0;      // 3-D slabs and 4-D ones sharded on z: the zero-extended synthesis exists
}

int ndwt_slab_halo(const ndwt_plan* p, int stride, int64_t* ab, int64_t* aa, int64_t* sb, int64_t* sa) {
    if (!p || stride < 1) return fail(NDWT_ERR_INVALID_ARG, "bad plan/stride");
    const int L = p->filt[p->shard].len;
    if (ab) *ab = (int64_t)(L / 2 - 1) * stride;
    if (aa) *aa = (int64_t)(L / 2) * stride;
    if (sb) *sb = (int64_t)(L / 2) * stride;
    if (sa) *sa = (int64_t)(L / 2 - 1) * stride;
    return NDWT_OK;
}

int ndwt_analysis_level_slab(ndwt_plan* p, const void* in, void* const* out, int stride, void* stream) {
    if (const int rb = refuse_batched(p, "a slab entry point")) return rb;
    if (!p || !in || !out || stride < 1) return fail(NDWT_ERR_INVALID_ARG, "bad arguments");
    return on_device(p, [&](auto t) { return analysis_level(p, (const decltype(t)*)in, (decltype(t)* const*)out, stride, true, (hipStream_t)stream); });
}

int ndwt_synthesis_level_slab(ndwt_plan* p, const void* const* in, void* out, int stride, void* stream) {
    if (const int rb = refuse_batched(p, "a slab entry point")) return rb;
    if (!p || !in || !out || stride < 1) return fail(NDWT_ERR_INVALID_ARG, "bad arguments");
    return on_device(p, [&](auto t) { return synthesis_level(p, (const decltype(t)* const*)in, (decltype(t)*)out, stride, true, kNoShrink, (hipStream_t)stream); });
}

int ndwt_analysis_level_slab_split(ndwt_plan* p, const void* in_local, const void* halo_before, const void* halo_after,
                                   void* const* out, int stride, void* stream) {
    if (p && p->shard != p->ndim - 1) {                  // z-slab: assembled with its halo planes, then the level (any plan kind)
        if (stride < 1) return fail(NDWT_ERR_INVALID_ARG, "bad stride");
        if (!in_local || !out || (p->filt[2].len > 2 && !halo_before) || !halo_after) return fail(NDWT_ERR_INVALID_ARG, "null pointer");
        return on_device(p, [&](auto t) { return slab_split_z_impl<decltype(t)>(p, in_local, halo_before, halo_after, out, stride, (hipStream_t)stream); });
    }
    // an outer-axis slab: every plane of it, as one part (a plan always has 1 <= dims[2] <= INT32_MAX planes)
    return ndwt_analysis_level_slab_part(p, in_local, halo_before, halo_after, out, stride, p ? p->dims[2] : 0, stream);
}

// what the split / extended forms of a fused 3-D slab plan check first: the plan (slab_fast_ok), then the two pointers each of them needs
static int slab_fast_begin(const ndwt_plan* p, int stride, int* Lp, const void* in, const void* out) {
    if (const int rc = slab_fast_ok(p, stride, Lp)) return rc;
    if (!in || !out) return fail(NDWT_ERR_INVALID_ARG, "null pointer");
    return NDWT_OK;
}

int ndwt_synthesis_level_slab_ext(ndwt_plan* p, const void* const* in_local, void* out_ext, int stride, void* stream) {
    int Lp = 0;
    if (p && p->shard != p->ndim - 1) {                  // z-sharded 4-D: the fused kernels with the z filter the longest, tap stride 1
        if (stride != 1 || !(Lp = slab_fused3(sel(p), 1, 1, kSlabZ)))
            return fail(NDWT_ERR_UNSUPPORTED, "the zero-extended z-slab synthesis needs a plan on the fused 3-D kernels whose z filter is the longest (stride 1)");
        if (!in_local || !out_ext) return fail(NDWT_ERR_INVALID_ARG, "null pointer");
        return on_device(p, [&](auto t) { return slab_ext_z_impl<decltype(t)>(p, Lp, in_local, out_ext, (hipStream_t)stream); });
    }
    if (p && p->ndim == 4) {                             // t-sharded 4-D: 3-D part per frame, zero-extended t-axis pass
        const LevelRoute r = level_route(sel(p), 1, -1, kSlabOuter);
        Lp = r.Lp;
        if (stride != 1 || r.kind != kRouteFused3T)
            return fail(NDWT_ERR_UNSUPPORTED, "the zero-extended 4-D slab synthesis needs a plan on the fused 3-D kernels (stride 1)");
        if (!in_local || !out_ext) return fail(NDWT_ERR_INVALID_ARG, "null pointer");
        return on_device(p, [&](auto t) { return slab_ext4_impl<decltype(t)>(p, Lp, in_local, out_ext, (hipStream_t)stream); });
    }
    if (const int rc = slab_fast_begin(p, stride, &Lp, in_local, out_ext)) return rc;
    return on_device(p, [&](auto t) { return slab_ext_impl<decltype(t)>(p, Lp, in_local, out_ext, (hipStream_t)stream); });
}

int ndwt_analysis_level_slab_part(ndwt_plan* p, const void* in_local, const void* halo_before, const void* halo_after,
                                  void* const* out, int stride, int64_t n_planes, void* stream) {
    int Lp = 0;
    int rc = slab_fast_ok(p, stride, &Lp);
    if (rc) return rc;
    if (!in_local || !out || (Lp > 2 && !halo_before) || !halo_after) return fail(NDWT_ERR_INVALID_ARG, "null pointer");
    if (n_planes < 1 || n_planes > INT32_MAX) return fail(NDWT_ERR_INVALID_ARG, "n_planes must be >= 1");
    if (!halo_before) halo_before = halo_after;          // db1: no plane before the slab is needed
    return on_device(p, [&](auto t) {
        return slab_analysis_part_impl<decltype(t)>(p, Lp, in_local, halo_before, halo_after, out, n_planes, (hipStream_t)stream);
    });
}

int ndwt_synthesis_level_slab_runs(ndwt_plan* p, const void* const* in_local, int64_t n_in, int64_t e0, int64_t e_stride,
                                   int64_t n_runs, int64_t n_out, void* out, int stride, void* stream) {
    int Lp = 0;
    if (const int rc = slab_fast_begin(p, stride, &Lp, in_local, out)) return rc;
    if (n_in < 1 || e0 < 0 || n_out < 1 || n_runs < 1 || e_stride < 0 || n_in > INT32_MAX ||
        e0 + (n_runs - 1) * e_stride + n_out > n_in + Lp - 1)
        return fail(NDWT_ERR_INVALID_ARG, "every run of output planes must lie inside the %lld planes of the zero-extended result",
                    (long long)(n_in + Lp - 1));
    return on_device(p, [&](auto t) {
        return slab_synthesis_runs_impl<decltype(t)>(p, Lp, in_local, n_in, e0, e_stride, n_runs, n_out, out, (hipStream_t)stream);
    });
}

int ndwt_synthesis_level_slab_part(ndwt_plan* p, const void* const* in_local, int64_t n_in, int64_t e0, int64_t n_out,
                                   void* out, int stride, void* stream) {
    return ndwt_synthesis_level_slab_runs(p, in_local, n_in, e0, 0, 1, n_out, out, stride, stream);
}

int ndwt_analysis_level_slab_runs(ndwt_plan* p, const void* in_with_halo, void* const* out, int stride, int64_t n_planes,
                                  int64_t n_runs, int64_t run_stride, void* stream) {
    int Lp = 0;
    if (const int rc = slab_fast_begin(p, stride, &Lp, in_with_halo, out)) return rc;
    if (n_planes < 1 || n_planes > INT32_MAX || n_runs < 1 || run_stride < 0) return fail(NDWT_ERR_INVALID_ARG, "bad run geometry");
    return on_device(p, [&](auto t) {
        return slab_analysis_runs_impl<decltype(t)>(p, Lp, in_with_halo, out, n_planes, n_runs, run_stride, (hipStream_t)stream);
    });
}

#ifdef NDWT_STAMPS
// diagnostic builds only (tools/stamps_inv.py): 4 cycle sums per wave of every workgroup of the next synthesis launches
int ndwt_plan_set_stamps(ndwt_plan* p, void* dev_buffer) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    p->stamps = (long long*)dev_buffer;
    return NDWT_OK;
}
#endif

const char* ndwt_last_error(void) { return g_last_error.c_str(); }
// what both segment forms check first
static int segments_check(const ndwt_plan* p, int op, int nseg) {
    if (!p) return fail(NDWT_ERR_INVALID_ARG, "null plan");
    if (const int rb = refuse_batched(p, "ndwt_slab_segments")) return rb;
    if (op != NDWT_SEG_COPY && op != NDWT_SEG_ADD) return fail(NDWT_ERR_INVALID_ARG, "op must be NDWT_SEG_COPY or NDWT_SEG_ADD");
    if (nseg < 0 || nseg > NDWT_MAX_SEGMENTS) return fail(NDWT_ERR_INVALID_ARG, "at most %d runs per call", NDWT_MAX_SEGMENTS);
    return NDWT_OK;
}
static int segments_launched(int rc) {
    return rc == 0 ? NDWT_OK : fail(NDWT_ERR_HIP, "segment kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
}

int ndwt_slab_segments(ndwt_plan* p, int op, int nseg, void* const* dst, const void* const* src, const int64_t* count, void* stream) {
    if (const int rc = segments_check(p, op, nseg)) return rc;
    if (nseg == 0) return NDWT_OK;
    if (!dst || !src || !count) return fail(NDWT_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < nseg; ++i)
        if (!dst[i] || !src[i] || count[i] < 0) return fail(NDWT_ERR_INVALID_ARG, "run %d: null pointer or negative count", i);
    return on_device(p, [&](auto t) { return segments_launched(segments_launch<decltype(t)>(op, nseg, dst, src, count, (hipStream_t)stream)); });
}

int ndwt_slab_segments_strided(ndwt_plan* p, int op, int nseg, void* const* dst, const void* const* src, const int64_t* count, int64_t nrep,
                               const int64_t* dst_stride, const int64_t* src_stride, void* stream) {
    if (const int rc = segments_check(p, op, nseg)) return rc;
    if (nrep < 0) return fail(NDWT_ERR_INVALID_ARG, "negative repetition count");
    if (nseg == 0 || nrep == 0) return NDWT_OK;
    if (!dst || !src || !count || !dst_stride || !src_stride) return fail(NDWT_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < nseg; ++i) {
        if (!dst[i] || !src[i] || count[i] < 0 || dst_stride[i] < 0 || src_stride[i] < 0)
            return fail(NDWT_ERR_INVALID_ARG, "run %d: null pointer, negative count or negative stride", i);
        if (nrep > 1 && dst_stride[i] < count[i])      // the repetitions of a run are written concurrently: they must not overlap
            return fail(NDWT_ERR_INVALID_ARG, "run %d: destination stride %lld is shorter than the run (%lld)", i, (long long)dst_stride[i],
                        (long long)count[i]);
    }
    return on_device(p, [&](auto t) {
        return segments_launched(segments_strided_launch<decltype(t)>(op, nseg, dst, src, count, nrep, dst_stride, src_stride, (hipStream_t)stream));
    });
}

const char* ndwt_version(void) { return "ndwt-hip 0.1 (gfx950)"; }

int ndwt_trace_enable(int on) {
    std::lock_guard<std::mutex> lk(g_trace_mu);
    const int was = g_trace_on.load(std::memory_order_relaxed);
    if (on) g_trace_log.clear();
    g_trace_on.store(on ? 1 : 0, std::memory_order_relaxed);
    return was;
}

int ndwt_trace_get(char* buf, int buflen) {
    std::lock_guard<std::mutex> lk(g_trace_mu);
    const size_t need = g_trace_log.size() + 1;
    if (buf && buflen > 0) {
        const size_t n = need <= (size_t)buflen ? need - 1 : (size_t)buflen - 1;
        memcpy(buf, g_trace_log.data(), n);
        buf[n] = 0;
    }
    return need > (size_t)INT_MAX ? INT_MAX : (int)need;
}

}  // extern "C"
