// The host launch toolkit.  For the propagator units (thz_asm.hip, thz_rsc.hip, thz_czt.hip,
// thz_f64.hip): the list of instantiated transform sizes and its dispatchers, workgroup sizes, the
// large-LDS opt-in.  For every unit, the add-on units (noise, losses, heightmap, metrics, ifta,
// optics) included: the workspace alignment and check and the pointer checks (misaligned,
// check_arrays, all_aligned16).  Host code only; include after thz_common.hpp.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <type_traits>
#include <vector>

namespace thz {

// ---- the instantiated sizes ------------------------------------------------------------------
// The one list of compile-time power-of-two transform lengths (blockDim = n / FFT_MAXV); the
// mixed-radix lengths are Mx300 / Mx500 (is_mx, MxOf; thz_asm.hip) and every other length runs the
// runtime plan (the <0> instantiation).  A dispatcher calls f(Size<N>{}) for the instantiation that
// serves n, so `KER<N()>` inside a generic lambda names the kernel; one dispatcher per kind of
// kernel family.
template <int N>
using Size = std::integral_constant<int, N>;
template <int... Ns>
struct SizeList {};
using Pow2Sizes = SizeList<1024, 2048, 4096, 8192, 16384>;

template <class F, int... Ns>
static bool on_listed(SizeList<Ns...>, int n, F&& f) {
  return ((n == Ns ? (f(Size<Ns>{}), true) : false) || ...);
}
template <class F, int... Ns>
static void for_each_size(SizeList<Ns...>, F&& f) {
  (f(Size<Ns>{}), ...);
}
// families that exist for the compile-time powers of two only (the z-x slice column passes):
// false when n is none of them
template <class F>
static bool on_pow2_only(int n, F&& f) {
  return on_listed(Pow2Sizes{}, n, f);
}
// families with a runtime-plan instantiation behind the powers of two (asm_cols, asm_rows_slice,
// fft_rows_kernel, the RSC and CZT transforms)
template <class F>
static void on_pow2(int n, F&& f) {
  if (!on_listed(Pow2Sizes{}, n, f)) f(Size<0>{});
}

static int pow2_kind(int n) { return on_pow2_only(n, [](auto) {}) ? n : 0; }
// workgroup size of the power-of-two / runtime-plan families
static int threads_for(int n) { return pow2_kind(n) ? n / pow2_v(n) : fft_threads(n); }

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static int check_workspace(const void* workspace, size_t bytes, size_t need) {
  if (!workspace || bytes < need) return fail(THZ_E_WORKSPACE, "workspace %zu bytes < required %zu", bytes, need);
  return THZ_OK;
}

// ---- pointer checks (host only, before any device call) --------------------------------------
static bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// every array present and aligned to its element
static int check_arrays(const char* who, std::initializer_list<const void*> ptrs, size_t elem) {
  for (const void* p : ptrs) {
    if (!p) return fail(THZ_E_ARG, "%s: null pointer", who);
    if (misaligned(p, elem)) return fail(THZ_E_ARG, "%s: array not %zu-byte aligned", who, elem);
  }
  return THZ_OK;
}

// the pointer half of a kernel's 16-byte form; a null pointer (an absent optional array) is aligned
static bool all_aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (misaligned(p, 16)) return false;
  return true;
}

// Workgroups above 64 KiB of dynamic LDS must opt in once per kernel.  Each kernel family keeps a
// once-guarded function that lists its instantiations (for_each_size(Pow2Sizes{}, ...) plus
// Size<0>) and names the largest byte count it launches with; the first error is reported.
static int lds_opt_in(const std::vector<const void*>& kernels, size_t bytes) {
  for (const void* k : kernels) {
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(THZ_E_HIP, "large-LDS opt-in (%zu bytes): %s", bytes, hipGetErrorString(e));
  }
  return THZ_OK;
}

}  // namespace thz
