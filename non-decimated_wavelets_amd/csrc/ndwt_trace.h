// ndwt_trace.h -- host-side launch trace (include/ndwt.h: ndwt_trace_enable / ndwt_trace_get).
//
// Every kernel launch site calls one of the helpers below right before its hipLaunchKernelGGL.  With the trace off (the default)
// that costs one relaxed atomic load; with it on, a record "<kernel type> grid=(x,y,z) block=(x,y,z)" is appended to a process-global
// log under a mutex (launches of the multi-device worker threads included).  Host-side only: nothing changes in what is launched, so
// results and graph capture are unaffected.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

namespace ndwt {

extern std::atomic<int> g_trace_on;
inline bool trace_on() { return g_trace_on.load(std::memory_order_relaxed) != 0; }

// appends one record; `kernel` is the type text (no newline)
void trace_append(const std::string& kernel, dim3 grid, dim3 block);
// the text of K out of __PRETTY_FUNCTION__ of trace_type_name<K>() ("... [K = ndwt::Fwd3<float, 8, ...>]"); note that clang leaves
// out trailing template arguments equal to their defaults
void trace_append_pretty(const char* pretty, dim3 grid, dim3 block);

template <class K> const char* trace_type_name() { return __PRETTY_FUNCTION__; }

// a launch of fused3_kernel<K> / march_kernel<K>: the record names K
template <class K> inline void trace_kernel(dim3 grid, dim3 block) {
    if (trace_on()) trace_append_pretty(trace_type_name<K>(), grid, block);
}

// a plain __global__ template: name<args...> spelled out by the launch site
inline void trace_arg(std::string& s, const char* v) { s += v; }
inline void trace_arg(std::string& s, bool v) { s += v ? "true" : "false"; }
inline void trace_arg(std::string& s, int v) { s += std::to_string(v); }
template <class T> constexpr const char* trace_scalar() { return sizeof(T) == 4 ? "float" : "double"; }

template <class... A> inline void trace_plain(dim3 grid, dim3 block, const char* name, A... args) {
    if (!trace_on()) return;
    std::string s = std::string("ndwt::") + name;
    if (sizeof...(args)) {
        s += "<";
        int i = 0;
        ((s += (i++ ? ", " : ""), trace_arg(s, args)), ...);
        s += ">";
    }
    trace_append(s, grid, block);
}

}  // namespace ndwt
