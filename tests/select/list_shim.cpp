// The instance lists of csrc/ndwt_fused_list.h, spelled as the launch trace spells a launch: one line per listed instance, "Family K=V ..".
// For tests/test_gpu_small_taps.py, which must run every listed single-precision instance of 10 taps or more (host C++ only:
// g++ -std=c++17 -shared -fPIC).  A tile number V becomes the tile's TY / NT / RY (csrc/ndwt_fused_tile.h), as the trace has no V.
#include <string>
#include "../../non-decimated_wavelets_amd/csrc/ndwt_select.h"
using namespace ndwt;

static std::string g_out;
static const char* tn(bool f64) { return f64 ? "double" : "float"; }
static const char* bs(bool b) { return b ? "true" : "false"; }
static void kv(const char* k, int v) { g_out += std::string(" ") + k + "=" + std::to_string(v); }
static void kv(const char* k, const char* v) { g_out += std::string(" ") + k + "=" + v; }
template <typename T> struct is64 { static constexpr bool value = sizeof(T) == 8; };

static void fused3(const char* fam, Fused3Kernel kernel, bool f64, int L, int V, bool vec4, int ew) {
    const TileShape t = fused3_tile_shape(kernel, f64, V, L, ew);
    g_out += fam;
    kv("T", tn(f64)); kv("L", L); kv("TX", t.TX); kv("TY", t.TY); kv("NT", t.NT); kv("RY", t.RY); kv("VEC4", bs(vec4)); kv("EW", ew);
}
#define LIST_F(T, L, V, VEC4, EW, PIN, TPRE, WLDS) \
    fused3("Fwd3", kFwd3, is64<T>::value, L, V, VEC4, EW); kv("PIN", bs(PIN)); kv("TPRE", bs(TPRE)); kv("WLDS", WLDS); g_out += "\n";
#define LIST_S(KIND, T, L, V, VEC4, EW) fused3(#KIND, k##KIND, is64<T>::value, L, V, VEC4, EW); g_out += "\n";
#define LIST_Y(L, VEC4, EW, DEPTH, UNIYZ, XSC) \
    g_out += "Inv3Y"; kv("T", "float"); kv("L", L); kv("TX", inv3y_tx(L, EW)); kv("TY", inv3y_ty(L, EW)); kv("VEC4", bs(VEC4)); kv("EW", EW); \
    kv("DEPTH", DEPTH); kv("ZLDS", inv3y_zlds(L, DEPTH, EW)); kv("UNIYZ", bs(UNIYZ)); kv("XSC", bs(XSC)); g_out += "\n";
#define LIST_W(KIND, T, L, VEC4, WPE, EW) \
    g_out += #KIND; kv("T", tn(is64<T>::value)); kv("L", L); kv("VEC4", bs(VEC4)); kv("WPE", WPE); kv("EW", EW); g_out += "\n";
#define LIST_P(T, L, PD, PK) g_out += "Inv2P"; kv("T", tn(is64<T>::value)); kv("L", L); kv("PD", PD); kv("PK", bs(PK)); g_out += "\n";
#define LIST_A(T, EW, L, NLEV, WPE) \
    g_out += "Fwd2C"; kv("T", tn(is64<T>::value)); kv("L", L); kv("NLEV", NLEV); kv("WPE", WPE); kv("EW", EW); g_out += "\n";
#define LIST_R(T, EW, L, NLEV, PD, WPE) \
    g_out += "Inv2C"; kv("T", tn(is64<T>::value)); kv("L", L); kv("NLEV", NLEV); kv("PD", PD); kv("WPE", WPE); kv("EW", EW); g_out += "\n";
#define LIST_N(T, L, SYN) g_out += "AxisMarch"; kv("T", tn(is64<T>::value)); kv("L", L); kv("SYN", bs(SYN)); g_out += "\n";
#define LIST_X(T, L, SYN, EW, VEC4) \
    g_out += "AxisX"; kv("T", tn(is64<T>::value)); kv("L", L); kv("SYN", bs(SYN)); kv("EW", EW); kv("VEC4", bs(VEC4)); g_out += "\n";

// every listed instance of the fused 3-D and 2-D kernels, the 2-D cascade and the per-axis passes; the text lives until the next call
extern "C" const char* list_instances() {
    g_out.clear();
    NDWT_LIST_F32_FWD(LIST_F) NDWT_LIST_F32_FWDP(LIST_F) NDWT_LIST_F32_DEN(LIST_F) NDWT_LIST_F32_LONG(LIST_F) NDWT_LIST_F32_LONGB(LIST_F)
    NDWT_LIST_F32_INV(LIST_S) NDWT_LIST_F32_INVE(LIST_S) NDWT_LIST_F32_LONGI(LIST_S)
    NDWT_LIST_F64_FWD(LIST_F) NDWT_LIST_F64_INV(LIST_S) NDWT_LIST_F64_LONG(LIST_F, LIST_S)
    NDWT_LIST_F32_INVY(LIST_Y) NDWT_LIST_F32_INVYS(LIST_Y) NDWT_LIST_F32_INVYC(LIST_Y)
    NDWT_LIST_2S(LIST_W, Fwd2S) NDWT_LIST_2S(LIST_W, Inv2S)
    NDWT_LIST_F32_INV2P(LIST_P) NDWT_LIST_F64_INV2P(LIST_P)
    NDWT_LIST_F32_FWD2C(LIST_A) NDWT_LIST_C64_FWD2C(LIST_A) NDWT_LIST_F64_FWD2C(LIST_A) NDWT_LIST_C128_FWD2C(LIST_A)
    NDWT_LIST_F32_INV2C(LIST_R) NDWT_LIST_C64_INV2C(LIST_R) NDWT_LIST_F64_INV2C(LIST_R) NDWT_LIST_C128_INV2C(LIST_R)
    NDWT_LIST_F32_AXIS_MARCH(LIST_N) NDWT_LIST_F64_AXIS_MARCH(LIST_N)
    NDWT_LIST_F32_AXISX(LIST_X) NDWT_LIST_F64_AXISX(LIST_X)
    return g_out.c_str();
}
