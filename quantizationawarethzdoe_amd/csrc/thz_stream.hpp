// The streaming toolkit of the add-on units (thz_noise.hip, thz_losses.hip, thz_heightmap.hip,
// thz_metrics.hip, thz_ifta.hip and the polarization kernels of thz_optics.hip): the four-element
// mover and the lane built on it, the fixed-order workgroup reduction, and the partials-then-finish
// sums.  No propagator unit includes it.  The MSE loss sink (thz_dev.hpp) keeps its own reduction.
#pragma once
#include <hip/hip_runtime.h>

namespace thz {

// ---------------------------------------------------------------------------------------------
// Four consecutive elements p[i .. i + 3] of an array of n: 16-byte accesses (one for a 4-byte T, two
// for an 8-byte, four for a 16-byte) when `wide` and the group lies inside n, else element accesses
// under a bound check, zero past the end -- the same values in the same lane either way.  The caller
// passes wide only where p + i is 16-byte aligned: an aligned base, and rows of a length that keeps
// every row's start aligned.  T: float, int, float2, double, double2.
// ---------------------------------------------------------------------------------------------
// The 4-byte types and float2 move as float4 / int4 values, component by component: the access then
// carries the array's own type, and the compiler knows that a store to a float array leaves a kernel's
// unsigned operands alone (moved as untyped words, the noise kernels re-read the generator's state with
// vector loads after every store: +12 % on the Gaussian and uniform kernels).
template <class T, class V>
__device__ __forceinline__ void ld4_as(const T* p, long long i, long long n, bool wide, T v[4]) {
  if (wide && i + 3 < n) {
    const V f = *reinterpret_cast<const V*>(p + i);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? p[i + k] : T{};
  }
}
template <class T, class V>
__device__ __forceinline__ void st4_as(T* p, long long i, long long n, bool wide, const T v[4]) {
  if (wide && i + 3 < n) {
    V f;
    f.x = v[0]; f.y = v[1]; f.z = v[2]; f.w = v[3];
    *reinterpret_cast<V*>(p + i) = f;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) p[i + k] = v[k];
  }
}
__device__ __forceinline__ void ld4(const float* p, long long i, long long n, bool wide, float v[4]) {
  ld4_as<float, float4>(p, i, n, wide, v);
}
__device__ __forceinline__ void ld4(const int* p, long long i, long long n, bool wide, int v[4]) {
  ld4_as<int, int4>(p, i, n, wide, v);
}
__device__ __forceinline__ void st4(float* p, long long i, long long n, bool wide, const float v[4]) {
  st4_as<float, float4>(p, i, n, wide, v);
}
__device__ __forceinline__ void st4(int* p, long long i, long long n, bool wide, const int v[4]) {
  st4_as<int, int4>(p, i, n, wide, v);
}
__device__ __forceinline__ void ld4(const float2* p, long long i, long long n, bool wide, float2 v[4]) {
  if (wide && i + 3 < n) {
    const float4* q = reinterpret_cast<const float4*>(p + i);
    const float4 f0 = q[0], f1 = q[1];
    v[0] = make_float2(f0.x, f0.y); v[1] = make_float2(f0.z, f0.w);
    v[2] = make_float2(f1.x, f1.y); v[3] = make_float2(f1.z, f1.w);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? p[i + k] : make_float2(0.f, 0.f);
  }
}
__device__ __forceinline__ void st4(float2* p, long long i, long long n, bool wide, const float2 v[4]) {
  if (wide && i + 3 < n) {
    float4* q = reinterpret_cast<float4*>(p + i);
    q[0] = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
    q[1] = make_float4(v[2].x, v[2].y, v[3].x, v[3].y);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) p[i + k] = v[k];
  }
}
// double, double2: two or four 16-byte words
template <class T>
__device__ __forceinline__ void ld4(const T* p, long long i, long long n, bool wide, T v[4]) {
  if (wide && i + 3 < n) {
    constexpr int NQ = (int)(sizeof(T) * 4 / 16);
    uint4 raw[NQ];
    const uint4* q = reinterpret_cast<const uint4*>(p + i);
#pragma unroll
    for (int m = 0; m < NQ; ++m) raw[m] = q[m];
    __builtin_memcpy(v, raw, sizeof(raw));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? p[i + k] : T{};
  }
}
template <class T>
__device__ __forceinline__ void st4(T* p, long long i, long long n, bool wide, const T v[4]) {
  if (wide && i + 3 < n) {
    constexpr int NQ = (int)(sizeof(T) * 4 / 16);
    uint4 raw[NQ];
    __builtin_memcpy(raw, v, sizeof(raw));
    uint4* q = reinterpret_cast<uint4*>(p + i);
#pragma unroll
    for (int m = 0; m < NQ; ++m) q[m] = raw[m];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) p[i + k] = v[k];
  }
}

// ---------------------------------------------------------------------------------------------
// The lane of a 16-byte streaming kernel: four elements per lane per round of a grid-stride loop over
// chunks of LANE_CHUNK.  WIDE: the lane's four are consecutive and move through ld4 / st4 (the host
// picks WIDE only when every pointer is 16-byte aligned; callers that index rows of length m into the
// arrays also need m % 4 == 0, so that every row starts aligned -- a flat array does not); otherwise
// element-width accesses, the lane's elements a workgroup apart (coalesced).  A group that crosses n
// moves element by element under a bound check in either form, which is what serves a flat n with
// n % 4 != 0.  at(k) is the element index of the lane's k-th value.  wide = false keeps the WIDE
// lane's four consecutive elements and moves them at element width (sum_lane).
// ---------------------------------------------------------------------------------------------
constexpr int LANE_THREADS = 256;
constexpr int LANE_PX = 4;  // elements per lane per round
constexpr int LANE_CHUNK = LANE_THREADS * LANE_PX;

template <bool WIDE>
struct Lane4 {
  long long p0, n;
  bool wide;
  __device__ __forceinline__ Lane4(long long c0, long long n_, bool wide_ = true) : n(n_), wide(WIDE && wide_) {
    p0 = c0 + (WIDE ? LANE_PX * (long long)threadIdx.x : (long long)threadIdx.x);
  }
  __device__ __forceinline__ long long at(int k) const { return p0 + (WIDE ? k : k * LANE_THREADS); }
  template <class T>
  __device__ __forceinline__ void load(const T* __restrict__ a, T v[LANE_PX]) const {
    if (WIDE) {
      ld4(a, p0, n, wide, v);
    } else {
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k) v[k] = at(k) < n ? a[at(k)] : T{};
    }
  }
  template <class T>
  __device__ __forceinline__ void store(T* __restrict__ a, const T v[LANE_PX]) const {
    if (WIDE) {
      st4(a, p0, n, wide, v);
    } else {
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k)
        if (at(k) < n) a[at(k)] = v[k];
    }
  }
};

// The lane of a sum: four consecutive values whether or not they move as one 16-byte access (`wide`:
// 16-byte aligned base and rows), so a sum's bits depend on the values only, not on the alignment of
// the arrays.
__device__ __forceinline__ Lane4<true> sum_lane(long long c0, long long m, bool wide) {
  return Lane4<true>(c0, m, wide);
}

// ---------------------------------------------------------------------------------------------
// Workgroup reduction in a fixed order: xor butterfly with offsets 32 .. 1 inside a wave, lane 0 of
// each wave to LDS, then thread 0 merges waves 1 .. nw - 1 in index order.  The result is valid in
// thread 0; every thread must call it.  Acc offers merge(const Acc&) and shfl_xor(offset), its own
// fields taken from the lane `offset` away.  Each field sees the operations of a reduction of its own
// in the same order, so an accumulator of K fields gives the bits of K separate reductions.
// ---------------------------------------------------------------------------------------------
template <class Acc>
__device__ __forceinline__ Acc block_reduce_fixed(Acc a) {
  __shared__ Acc s_w[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  for (int o = 32; o > 0; o >>= 1) a.merge(a.shfl_xor(o));
  __syncthreads();
  if (lane == 0) s_w[wid] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < nw; ++w) a.merge(s_w[w]);
  return a;
}

// K fp64 sums
template <int K>
struct Sums {
  double v[K];
  __device__ __forceinline__ void merge(const Sums& o) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += o.v[k];
  }
  __device__ __forceinline__ Sums shfl_xor(int o) const {
    Sums r;
#pragma unroll
    for (int k = 0; k < K; ++k) r.v[k] = __shfl_xor(v[k], o);
    return r;
  }
};

// ---------------------------------------------------------------------------------------------
// Partials, then finish: a producing workgroup reduces its accumulator and thread 0 stores it in the
// workgroup's own slot (no atomics); a finish workgroup per item gathers the item's slots -- thread t
// takes slots t, t + blockDim, ... in ascending order -- and reduces again.  The grids depend on the
// shape alone, so a result's bits depend on the values only.
// ---------------------------------------------------------------------------------------------
constexpr int MAX_PARTS = 1024;  // workgroups of a partial-sum launch (4 per CU on an MI355X)

// slots per item: one per chunk of the item, the items together at most `cap`
inline int partial_parts(long long chunks, long long items = 1, long long cap = MAX_PARTS) {
  const long long each = items >= cap ? 1 : cap / items;
  return (int)(chunks < each ? chunks : each);
}

// every thread calls it; thread 0 stores
template <int K>
__device__ __forceinline__ void store_partials(const Sums<K>& a, double* __restrict__ partial, long long slot) {
  const Sums<K> r = block_reduce_fixed(a);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) partial[slot * K + k] = r.v[k];
  }
}

// add(i, acc) merges slot i into acc (and may skip it)
template <class Acc, class Add>
__device__ __forceinline__ Acc gather_reduce(Acc a, long long parts, Add add) {
  for (long long i = threadIdx.x; i < parts; i += blockDim.x) add(i, a);
  return block_reduce_fixed(a);
}
// the sums of slots first .. first + parts - 1
template <int K>
__device__ __forceinline__ Sums<K> gather_partials(const double* __restrict__ partial, long long parts,
                                                   long long first = 0) {
  const double* p = partial + first * K;
  return gather_reduce(Sums<K>{}, parts, [p](long long i, Sums<K>& a) {
#pragma unroll
    for (int k = 0; k < K; ++k) a.v[k] += p[i * K + k];
  });
}

}  // namespace thz
