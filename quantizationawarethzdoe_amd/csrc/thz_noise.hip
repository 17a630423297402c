// Detector noise models (Addons/Noise.py:4-112, utils/Noise.py:4-116, utils/Helper_Functions.py:
// 258-366) on the counter-based device generator (thz_dev.hpp: rng_bits; the samplers built on it are here).
//
//   thz_noise_apply         one streaming pass: reads the measurement (or the complex64 field, whose
//                           |E|^2 it forms in registers) and writes the noisy one -- 12 B per pixel for
//                           a field, 8 B for an intensity, against the ~60 B of the reference's seven
//                           elementwise passes and two RNG kernels.  The streaming lane of the Stokes
//                           kernels (Lane4): 16-byte accesses when the pointers and n allow, else the
//                           same body at element width; the arithmetic is per element and this unit
//                           compiles with contraction off, so both forms and every grid give the same bits.
//   thz_noise_draws         the raw draws of the same (state, stream, index), for tests.
//   thz_signal_scale        sqrt(mean |x|^2 / snr) into a device scalar: fp64 partial per workgroup,
//                           then one workgroup adds the partials in index order.
//   thz_snr_noise_backward  the cotangent of x + n scale(x): the same two-stage sum of Re(conj(g) n)
//                           with n regenerated, then one streaming pass gx = g + x coef.
// The two reductions give every lane four consecutive elements whether or not it can move them as one
// 16-byte access, and their grid depends on n alone, so a sum's bits depend on the values only.
#include <cstdint>
#include <initializer_list>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_stream.hpp"
#include "thz_launch.hpp"

#pragma clang fp contract(off)

namespace thz {

// ---------------------------------------------------------------------------------------------
// Detector-noise samplers (Addons/Noise.py:27,58,87-89, utils/Noise.py:32) on the counter-based
// generator of thz_dev.hpp: pure functions of (rng state, stream, element index, parameters), so a
// forward and its backward regenerate the same draw and a result never depends on the launch geometry
// or on what a neighbouring lane does.  fp32, contraction off.
// ---------------------------------------------------------------------------------------------
// The standard normals rng_normal2 / rng_normal (Box-Muller on two 24-bit uniforms of one rng_bits
// word, |n| <= 5.768) live next to rng_bits in thz_dev.hpp.
// complex standard normal, variance 1 in total (torch.randn of a complex dtype: 1/2 per component)
__device__ __forceinline__ float2 rng_cnormal(const unsigned* rng, unsigned stream, unsigned idx) {
  const float2 z = rng_normal2(rng, stream, idx);
  return make_float2(z.x * 0.70710678118654752f, z.y * 0.70710678118654752f);
}

// Poisson(lam) (torch.poisson), returned as a float.  lam = 0 gives 0; lam < 0 or NaN gives NaN (no
// host check: that would be a sync).  Rates up to 2^24 are supported (beyond it fp32 no longer holds
// every count); the tests cover 0.05 to 1e5.
//
// Attempt j of element idx draws word j of a splitmix64 sequence of its own, seeded with the
// element's base word rng_bits(state, stream ^ "POIS", idx): w_j = mix(base + (j + 1) gamma).  The
// attempt number enters the 64-bit counter in a hash round of its own and never the 32-bit stream,
// so (stream, j) pairs cannot alias: two streams' attempt sequences start from two hashed 64-bit
// words and meet only if those differ by a small multiple of gamma (probability ~2^-60 per pair).
// No w_j is the base word itself, so the Poisson draws of a stream are also apart from its normal /
// uniform draws, and a lane's sample does not depend on how long its neighbours loop.
//
// lam < 10: inversion by sequential search in fp64 on a 53-bit uniform (a 24-bit uniform could not
// reach the tail mass below 2^-24).  P(X >= 64 | lam < 10) < 4e-30, far below the uniform's 2^-53
// resolution, so the search bound of 64 only stops a cumulative sum that rounding left below u.
//
// lam >= 10: Hoermann's transformed rejection with squeeze (PTRS, Insurance: Mathematics and
// Economics 12 (1993) 39-45; the algorithm of numpy and of torch's CPU poisson), fp32.  U has 23
// bits and is centred ((b + 1/2) / 2^23 - 1/2, never 0 or +-1/2), V = (b + 1) / 2^24 in (0, 1].  An
// attempt accepts with probability 1 / invalpha: 0.75 at lam = 10, above 0.85 from lam = 90, 0.89
// in the limit; the squeeze alone (no log, no lgamma) accepts 0.35 - 0.80.  The loop runs until the
// lane accepts: there is no attempt cap, since returning early would bias the sample.
//
// The acceptance test compares with log pmf(k) = -lam + k log lam - lgamma(k + 1)
// (rng_poisson_logpmf).  Evaluated as written, with lgammaf, its terms are ~lam log lam and cancel
// to a few units: the result would carry 1e-3 absolute at lam = 1000 and 0.1 at 1e5.  So that form
// serves k < 16 only (small terms, or a candidate so far below lam that it is rejected whatever the
// rounding); from k = 16 Stirling's series for lgamma is folded in analytically, with d = k - lam
// and t = d / lam,
//   log pmf = -d t + k (t - log1p(t)) - log(2 pi k) / 2 - 1 / (12 k) + 1 / (360 k^3)   (+ < 1e-9),
// whose terms are of the size of d: ~1e-5 absolute at lam = 1000, ~1e-4 at 1e5.
constexpr unsigned RNG_POISSON_STREAM = 0x504F4953u;  // "POIS"
__device__ __forceinline__ unsigned long long rng_poisson_word(unsigned long long base, unsigned attempt) {
  unsigned long long x = base + ((unsigned long long)attempt + 1ull) * 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ float rng_poisson_logpmf(float k, float lam, float loglam) {
  if (k < 16.0f) return -lam + k * loglam - lgammaf(k + 1.0f);
  const float d = k - lam, t = d / lam, ik = 1.0f / k;
  return (-d * t + k * (t - log1pf(t))) - 0.5f * logf(6.2831853071795865f * k) -
         ik * (0.083333333333333333f - 0.0027777777777777778f * ik * ik);
}
__device__ inline float rng_poisson(const unsigned* rng, unsigned stream, unsigned idx, float lam) {
  if (!(lam >= 0.0f)) return __builtin_nanf("");
  if (lam == 0.0f) return 0.0f;
  const unsigned long long base = rng_bits(rng, stream ^ RNG_POISSON_STREAM, idx);
  if (lam < 10.0f) {
    const double u = (double)(rng_poisson_word(base, 0u) >> 11) * 0x1p-53;
    const double l = (double)lam;
    double p = exp(-l), s = p;
    int k = 0;
    while (u >= s && k < 64) {
      ++k;
      p *= l / (double)k;
      s += p;
    }
    return (float)k;
  }
  const float slam = sqrtf(lam), loglam = logf(lam);
  const float b = 0.931f + 2.53f * slam;
  const float a = -0.059f + 0.02483f * b;
  const float invalpha = 1.1239f + 1.1328f / (b - 3.4f);
  const float vr = 0.9277f - 3.6224f / (b - 2.0f);
  for (unsigned j = 0u;; ++j) {
    const unsigned long long w = rng_poisson_word(base, j);
    const float U = ((float)(unsigned)(w >> 41) + 0.5f) * (1.0f / 8388608.0f) - 0.5f;
    const float V = (float)(((unsigned)(w >> 16) & 0xFFFFFFu) + 1u) * (1.0f / 16777216.0f);
    const float us = 0.5f - fabsf(U);
    const float k = floorf((2.0f * a / us + b) * U + lam + 0.43f);
    if (us >= 0.07f && V <= vr) return k;
    if (k < 0.0f || (us < 0.013f && V > us)) continue;
    if (logf(V) + logf(invalpha) - logf(a / (us * us) + b) <= rng_poisson_logpmf(k, lam, loglam)) return k;
  }
}

struct NoiseArgs {
  float sigma, a, gain;
  int normalize;
  const float* sigma_dev;
  const unsigned* rng;
  unsigned stream;
};

// one element of the four models, in the reference's operation order (Addons/Noise.py:27, 58-61, 87-89, 112)
template <int KIND>
__device__ __forceinline__ float noise_model(float x, unsigned idx, const NoiseArgs& p, float sigma) {
  if (KIND == THZ_NOISE_GAUSS) return x + rng_normal(p.rng, p.stream, idx) * sigma;
  if (KIND == THZ_NOISE_UNIFORM) return x + ((rng_u01(p.rng, p.stream, idx) - 0.5f) * 2.0f) * p.a;
  const float counts = rng_poisson(p.rng, p.stream, idx, x / p.gain);
  if (KIND == THZ_NOISE_POISSON) return p.normalize ? counts * p.gain : counts;
  return counts * p.gain + rng_normal(p.rng, p.stream, idx) * sigma;
}

template <int KIND, int INPUT, bool WIDE>
__global__ void __launch_bounds__(LANE_THREADS) noise_apply_kernel(const void* __restrict__ in, void* __restrict__ out,
                                                                  long long n, NoiseArgs p) {
  const float sigma = p.sigma_dev ? *p.sigma_dev : p.sigma;
  for (long long c0 = (long long)blockIdx.x * LANE_CHUNK; c0 < n; c0 += (long long)gridDim.x * LANE_CHUNK) {
    const Lane4<WIDE> L(c0, n);
    if (INPUT == THZ_NOISE_IN_COMPLEX64) {
      float2 v[LANE_PX];
      L.load((const float2*)in, v);
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k) {
        if (L.at(k) >= n) continue;
        const float2 z = rng_cnormal(p.rng, p.stream, (unsigned)L.at(k));
        v[k] = make_float2(v[k].x + z.x * sigma, v[k].y + z.y * sigma);
      }
      L.store((float2*)out, v);
    } else {
      float x[LANE_PX];
      if (INPUT == THZ_NOISE_IN_FIELD_INTENSITY) {
        float2 e[LANE_PX];
        L.load((const float2*)in, e);
#pragma unroll
        for (int k = 0; k < LANE_PX; ++k) x[k] = loss_intensity(e[k]);  // field.abs() ** 2
      } else {
        L.load((const float*)in, x);
      }
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k)
        if (L.at(k) < n) x[k] = noise_model<KIND>(x[k], (unsigned)L.at(k), p, sigma);
      L.store((float*)out, x);
    }
  }
}

__global__ void __launch_bounds__(LANE_THREADS) noise_draws_kernel(int what, const unsigned* __restrict__ rng,
                                                                  unsigned stream, long long n,
                                                                  float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * LANE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * LANE_THREADS) {
    if (what == THZ_DRAW_NORMAL) {
      out[i] = rng_normal(rng, stream, (unsigned)i);
    } else if (what == THZ_DRAW_UNIFORM) {
      out[i] = rng_u01(rng, stream, (unsigned)i);
    } else {
      const float2 z = rng_cnormal(rng, stream, (unsigned)i);
      out[2 * i] = z.x;
      out[2 * i + 1] = z.y;
    }
  }
}

// ---- the two-stage fp64 sums (thz_stream.hpp) ------------------------------------------------
static int sum_parts(long long elems) { return partial_parts((elems + LANE_CHUNK - 1) / LANE_CHUNK); }
// workspace: the partials, then the backward's coefficient (one float in its own 256 bytes)
static size_t sum_coef_offset() { return align256(sizeof(double) * MAX_PARTS); }
static size_t sum_workspace_bytes() { return sum_coef_offset() + 256; }

// partial[b] = sum over workgroup b's chunks of x_f^2, f over m floats (a complex array is its 2 n floats)
__global__ void __launch_bounds__(LANE_THREADS) signal_scale_part_kernel(const float* __restrict__ x, long long m,
                                                                        bool wide, double* __restrict__ partial) {
  double acc = 0.0;
  for (long long c0 = (long long)blockIdx.x * LANE_CHUNK; c0 < m; c0 += (long long)gridDim.x * LANE_CHUNK) {
    const Lane4<true> L = sum_lane(c0, m, wide);
    float v[LANE_PX];
    L.load(x, v);
#pragma unroll
    for (int k = 0; k < LANE_PX; ++k) acc += (double)v[k] * (double)v[k];
  }
  store_partials(Sums<1>{{acc}}, partial, blockIdx.x);
}

// scale = sqrt(mean |x|^2 / snr) (utils/Noise.py:28-32), rounded to fp32 once
__global__ void __launch_bounds__(LANE_THREADS) signal_scale_finish_kernel(const double* __restrict__ partial, int parts,
                                                                          double n, double snr,
                                                                          float* __restrict__ scale) {
  const double sum = gather_partials<1>(partial, parts).v[0];
  if (threadIdx.x == 0) *scale = (float)sqrt(sum / n / snr);
}

// partial[b] = sum of Re(conj(g_i) n_i) over workgroup b's chunks; n_i regenerated from (rng, stream, i).
// Real: a lane owns elements 4 t .. 4 t + 3 of its chunk; complex: the floats of elements 2 t, 2 t + 1.
template <bool CPLX>
__global__ void __launch_bounds__(LANE_THREADS) snr_noise_bwd_part_kernel(const float* __restrict__ g, long long m,
                                                                         bool wide, const unsigned* __restrict__ rng,
                                                                         unsigned stream, double* __restrict__ partial) {
  double acc = 0.0;
  for (long long c0 = (long long)blockIdx.x * LANE_CHUNK; c0 < m; c0 += (long long)gridDim.x * LANE_CHUNK) {
    const Lane4<true> L = sum_lane(c0, m, wide);
    float v[LANE_PX];
    L.load(g, v);
    if (CPLX) {
#pragma unroll
      for (int k = 0; k < LANE_PX; k += 2) {
        if (L.at(k) >= m) continue;
        const float2 z = rng_cnormal(rng, stream, (unsigned)(L.at(k) >> 1));
        acc += (double)v[k] * (double)z.x;
        acc += (double)v[k + 1] * (double)z.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k)
        if (L.at(k) < m) acc += (double)v[k] * (double)rng_normal(rng, stream, (unsigned)L.at(k));
    }
  }
  store_partials(Sums<1>{{acc}}, partial, blockIdx.x);
}

// coef = S / (N snr scale), rounded to fp32 once
__global__ void __launch_bounds__(LANE_THREADS) snr_noise_bwd_finish_kernel(const double* __restrict__ partial,
                                                                           int parts, double n, double snr,
                                                                           const float* __restrict__ scale,
                                                                           float* __restrict__ coef) {
  const double sum = gather_partials<1>(partial, parts).v[0];
  if (threadIdx.x == 0) *coef = (float)(sum / (n * snr * (double)*scale));
}

// gx = g + x coef over m floats
template <bool WIDE>
__global__ void __launch_bounds__(LANE_THREADS) snr_noise_bwd_kernel(const float* __restrict__ g,
                                                                    const float* __restrict__ x, long long m,
                                                                    const float* __restrict__ coef,
                                                                    float* __restrict__ gx) {
  const float c = *coef;
  for (long long c0 = (long long)blockIdx.x * LANE_CHUNK; c0 < m; c0 += (long long)gridDim.x * LANE_CHUNK) {
    const Lane4<WIDE> L(c0, m);
    float gv[LANE_PX], xv[LANE_PX];
    L.load(g, gv);
    L.load(x, xv);
#pragma unroll
    for (int k = 0; k < LANE_PX; ++k) gv[k] = gv[k] + xv[k] * c;
    L.store(gx, gv);
  }
}

// ---- host side -------------------------------------------------------------------------------
constexpr long long NOISE_MAX_N = 1LL << 32;  // the generator's element index is 32-bit

// the arrays, then the range of n, shared by the entries
static int noise_check(const char* who, std::initializer_list<const void*> ptrs, size_t elem, long long n) {
  if (int e = check_arrays(who, ptrs, elem)) return e;
  if (n < 0) return fail(THZ_E_ARG, "%s: n = %lld < 0", who, n);
  if (n > NOISE_MAX_N) return fail(THZ_E_ARG, "%s: n = %lld > 2^32, the generator's index range", who, n);
  return THZ_OK;
}

template <int KIND, int INPUT>
static void noise_apply_launch(bool wide, dim3 g, hipStream_t s, const void* in, void* out, long long n,
                               const NoiseArgs& p) {
  if (wide) hipLaunchKernelGGL((noise_apply_kernel<KIND, INPUT, true>), g, dim3(LANE_THREADS), 0, s, in, out, n, p);
  else hipLaunchKernelGGL((noise_apply_kernel<KIND, INPUT, false>), g, dim3(LANE_THREADS), 0, s, in, out, n, p);
}

template <int INPUT>
static void noise_apply_kind(int kind, bool wide, dim3 g, hipStream_t s, const void* in, void* out, long long n,
                             const NoiseArgs& p) {
  switch (kind) {
    case THZ_NOISE_GAUSS: return noise_apply_launch<THZ_NOISE_GAUSS, INPUT>(wide, g, s, in, out, n, p);
    case THZ_NOISE_UNIFORM: return noise_apply_launch<THZ_NOISE_UNIFORM, INPUT>(wide, g, s, in, out, n, p);
    case THZ_NOISE_POISSON: return noise_apply_launch<THZ_NOISE_POISSON, INPUT>(wide, g, s, in, out, n, p);
    default: return noise_apply_launch<THZ_NOISE_POISSON_GAUSS, INPUT>(wide, g, s, in, out, n, p);
  }
}

}  // namespace thz

using namespace thz;

extern "C" int thz_noise_apply(const thz_noise_desc* d, const void* in, void* out, long long n, thz_stream_t stream) {
  const char* who = "thz_noise_apply";
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->kind < THZ_NOISE_GAUSS || d->kind > THZ_NOISE_POISSON_GAUSS) return fail(THZ_E_ARG, "%s: kind %d", who, d->kind);
  if (d->input < THZ_NOISE_IN_REAL32 || d->input > THZ_NOISE_IN_COMPLEX64)
    return fail(THZ_E_ARG, "%s: input %d", who, d->input);
  if (d->input == THZ_NOISE_IN_COMPLEX64 && d->kind != THZ_NOISE_GAUSS)
    return fail(THZ_E_ARG, "%s: a complex64 output exists for the Gaussian kind only (kind %d)", who, d->kind);
  const bool cin = d->input != THZ_NOISE_IN_REAL32, cout = d->input == THZ_NOISE_IN_COMPLEX64;
  if (int e = noise_check(who, {in}, cin ? sizeof(float2) : sizeof(float), n)) return e;
  if (int e = noise_check(who, {out}, cout ? sizeof(float2) : sizeof(float), n)) return e;
  if (int e = noise_check(who, {d->rng}, sizeof(unsigned), n)) return e;
  if (d->sigma_dev && misaligned(d->sigma_dev, sizeof(float))) return fail(THZ_E_ARG, "%s: sigma_dev misaligned", who);
  const bool poisson = d->kind == THZ_NOISE_POISSON || d->kind == THZ_NOISE_POISSON_GAUSS;
  if (poisson && !(d->gain > 0.0f)) return fail(THZ_E_ARG, "%s: gain = %g must be positive", who, (double)d->gain);
  if (n == 0) return THZ_OK;
  hipStream_t s = (hipStream_t)stream;
  int blocks = 0;
  if (int e = stream_grid((n + LANE_CHUNK - 1) / LANE_CHUNK, &blocks)) return e;
  const NoiseArgs p{d->sigma, d->a, d->gain, d->normalize, d->sigma_dev, d->rng, d->stream};
  const bool wide = n % LANE_PX == 0 && all_aligned16({in, out});
  KernelTimer kt("noise_apply", s);
  const dim3 g((unsigned)blocks);
  if (d->input == THZ_NOISE_IN_COMPLEX64) noise_apply_launch<THZ_NOISE_GAUSS, THZ_NOISE_IN_COMPLEX64>(wide, g, s, in, out, n, p);
  else if (d->input == THZ_NOISE_IN_FIELD_INTENSITY) noise_apply_kind<THZ_NOISE_IN_FIELD_INTENSITY>(d->kind, wide, g, s, in, out, n, p);
  else noise_apply_kind<THZ_NOISE_IN_REAL32>(d->kind, wide, g, s, in, out, n, p);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_noise_draws(int what, const unsigned* rng, unsigned stream, long long n, float* out,
                               thz_stream_t stream_handle) {
  const char* who = "thz_noise_draws";
  if (what < THZ_DRAW_NORMAL || what > THZ_DRAW_COMPLEX_NORMAL) return fail(THZ_E_ARG, "%s: what = %d", who, what);
  if (int e = noise_check(who, {rng, out}, sizeof(float), n)) return e;
  if (n == 0) return THZ_OK;
  hipStream_t s = (hipStream_t)stream_handle;
  int blocks = 0;
  if (int e = stream_grid((n + LANE_THREADS - 1) / LANE_THREADS, &blocks)) return e;
  KernelTimer kt("noise_draws", s);
  hipLaunchKernelGGL(noise_draws_kernel, dim3((unsigned)blocks), dim3(LANE_THREADS), 0, s, what, rng, stream, n, out);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_signal_scale_workspace_size(long long n, size_t* bytes) {
  if (!bytes) return fail(THZ_E_ARG, "thz_signal_scale_workspace_size: null pointer");
  if (n < 0) return fail(THZ_E_ARG, "thz_signal_scale_workspace_size: n = %lld < 0", n);
  *bytes = sum_workspace_bytes();
  return THZ_OK;
}

extern "C" int thz_signal_scale(const void* x, long long n, int is_complex, float snr_linear, float* scale,
                                void* workspace, size_t bytes, thz_stream_t stream) {
  const char* who = "thz_signal_scale";
  if (int e = noise_check(who, {x}, is_complex ? sizeof(float2) : sizeof(float), n)) return e;
  if (int e = noise_check(who, {scale}, sizeof(float), n)) return e;
  if (int e = noise_check(who, {workspace}, sizeof(double), n)) return e;
  if (!(snr_linear > 0.0f)) return fail(THZ_E_ARG, "%s: snr_linear = %g must be positive", who, (double)snr_linear);
  if (n == 0) return THZ_OK;
  if (int e = check_workspace(workspace, bytes, sum_workspace_bytes())) return e;
  hipStream_t s = (hipStream_t)stream;
  const long long m = is_complex ? 2 * n : n;
  const int parts = sum_parts(m);
  double* partial = (double*)workspace;
  KernelTimer kp("signal_scale_part", s);
  hipLaunchKernelGGL(signal_scale_part_kernel, dim3((unsigned)parts), dim3(LANE_THREADS), 0, s, (const float*)x, m,
                     m % LANE_PX == 0 && all_aligned16({x}), partial);
  THZ_LAUNCH_CHECK();
  kp.stop();
  KernelTimer kf("signal_scale_finish", s);
  hipLaunchKernelGGL(signal_scale_finish_kernel, dim3(1), dim3(LANE_THREADS), 0, s, (const double*)partial, parts,
                     (double)n, (double)snr_linear, scale);
  THZ_LAUNCH_CHECK();
  kf.stop();
  return THZ_OK;
}

extern "C" int thz_snr_noise_backward(const void* g, const void* x, long long n, int is_complex, float snr_linear,
                                      const float* scale, const unsigned* rng, unsigned stream, void* gx,
                                      void* workspace, size_t bytes, thz_stream_t stream_handle) {
  const char* who = "thz_snr_noise_backward";
  if (int e = noise_check(who, {g, x, gx}, is_complex ? sizeof(float2) : sizeof(float), n)) return e;
  if (int e = noise_check(who, {scale, rng}, sizeof(float), n)) return e;
  if (int e = noise_check(who, {workspace}, sizeof(double), n)) return e;
  if (!(snr_linear > 0.0f)) return fail(THZ_E_ARG, "%s: snr_linear = %g must be positive", who, (double)snr_linear);
  if (n == 0) return THZ_OK;
  if (int e = check_workspace(workspace, bytes, sum_workspace_bytes())) return e;
  hipStream_t s = (hipStream_t)stream_handle;
  const long long m = is_complex ? 2 * n : n;
  const int parts = sum_parts(m);
  double* partial = (double*)workspace;
  float* coef = (float*)((char*)workspace + sum_coef_offset());
  const dim3 pg((unsigned)parts), b(LANE_THREADS);
  const bool gwide = m % LANE_PX == 0 && all_aligned16({g});
  KernelTimer kp("snr_noise_bwd_part", s);
  if (is_complex)
    hipLaunchKernelGGL(snr_noise_bwd_part_kernel<true>, pg, b, 0, s, (const float*)g, m, gwide, rng, stream, partial);
  else
    hipLaunchKernelGGL(snr_noise_bwd_part_kernel<false>, pg, b, 0, s, (const float*)g, m, gwide, rng, stream, partial);
  THZ_LAUNCH_CHECK();
  kp.stop();
  KernelTimer kf("snr_noise_bwd_finish", s);
  hipLaunchKernelGGL(snr_noise_bwd_finish_kernel, dim3(1), b, 0, s, (const double*)partial, parts, (double)n,
                     (double)snr_linear, scale, coef);
  THZ_LAUNCH_CHECK();
  kf.stop();
  int blocks = 0;
  if (int e = stream_grid((m + LANE_CHUNK - 1) / LANE_CHUNK, &blocks)) return e;
  KernelTimer ka("snr_noise_bwd", s);
  if (gwide && all_aligned16({x, gx}))
    hipLaunchKernelGGL(snr_noise_bwd_kernel<true>, dim3((unsigned)blocks), b, 0, s, (const float*)g, (const float*)x, m,
                       (const float*)coef, (float*)gx);
  else
    hipLaunchKernelGGL(snr_noise_bwd_kernel<false>, dim3((unsigned)blocks), b, 0, s, (const float*)g, (const float*)x,
                       m, (const float*)coef, (float*)gx);
  THZ_LAUNCH_CHECK();
  ka.stop();
  return THZ_OK;
}
