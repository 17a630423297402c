// Fabrication-tolerance Monte Carlo (include/thzdoe.h: thz_tolerance_*; tolerance.py): K perturbed
// realisations of one height map applied to one incident field.  The reference has one term of the
// model, add_height_map_noise's per-pixel U(-tol, tol) draw (Components/QuantizedDOE.py:82-87); the
// depth-scale and per-level terms are this port's.
//
//   thz_tolerance_modulate_forward   one streaming pass on the Lane4 lane of thz_stream.hpp: a workgroup
//                           takes a tile of TOL_KT realisations, puts their scale error and L level
//                           errors in LDS (16 x 17 draws, one per thread), then walks its chunks of
//                           field pixels; per chunk a lane loads its four map heights and level indices
//                           once and loops the tile's realisations innermost, so the field and map
//                           re-reads of a tile come from cache.  8 K C H W bytes written, 8 Bf C H W +
//                           4 hs ws (+ 4 hs ws of idx) read per tile.  heights_out is written in the same
//                           pass for a map of the field's size, by a small kernel of its own otherwise
//                           (an upsampled map has several, a downsampled one possibly no field pixel per
//                           map pixel).
//   thz_tolerance_modulate_backward  one thread per map pixel owns the field pixels that read it (the
//                           destination interval of the nearest upsampling, found by bisection on
//                           doe_nearest_src itself) and sums in fp64 in the order (c, q, k): no atomics,
//                           the same bits from every grid.  Every draw is regenerated per thread.
// Every draw is a pure function of (state, stream, k, p) and the unit compiles with contraction off, so
// both lane widths, every grid and every chunking of K give the same bits.
#include <climits>
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_stream.hpp"
#include "thz_launch.hpp"

#pragma clang fp contract(off)

namespace thz {

struct TolArgs {
  int K, Bf, C, H, W, hs, ws, L, rough_kind;
  int same;  // the map has the field's size: src(q) = q
  long long first;
  float sigma_scale, rough, lo, hi, eps, tand;
  const unsigned* rng;
  unsigned stream;
  float sigma_level[THZ_MAX_LUT];
  float lam[THZ_MAX_WAVELENGTHS];
};

// ---- the error model (thzdoe.h) ----------------------------------------------------------------
__device__ __forceinline__ float tol_scale(const TolArgs& a, long long k) {
  return a.sigma_scale != 0.0f ? a.sigma_scale * rng_normal(a.rng, a.stream ^ THZ_TOL_TAG_SCALE, (unsigned)k) : 0.0f;
}
// l in 0 .. THZ_MAX_LUT - 1
__device__ __forceinline__ float tol_level(const TolArgs& a, long long k, int l) {
  const float s = l < a.L ? a.sigma_level[l] : 0.0f;
  return s != 0.0f ? s * rng_normal(a.rng, a.stream ^ THZ_TOL_TAG_LEVEL, (unsigned)(16 * k + l)) : 0.0f;
}
__device__ __forceinline__ float tol_rough(const TolArgs& a, long long k, int p) {
  if (a.rough_kind == THZ_TOL_ROUGH_NONE || a.rough == 0.0f) return 0.0f;
  const unsigned i = (unsigned)(k * ((long long)a.hs * a.ws) + p);
  if (a.rough_kind == THZ_TOL_ROUGH_UNIFORM)
    return ((rng_u01(a.rng, a.stream ^ THZ_TOL_TAG_ROUGH, i) - 0.5f) * 2.0f) * a.rough;
  return a.rough * rng_normal(a.rng, a.stream ^ THZ_TOL_TAG_ROUGH, i);
}
// h_k[p]; *inside: the clamp passes the gradient (lo < u < hi)
__device__ __forceinline__ float tol_height(const TolArgs& a, float h, float g, float e, float r, bool* inside) {
  const float u = ((1.0f + g) * h + e) + r;
  if (inside) *inside = u > a.lo && u < a.hi;
  return fminf(fmaxf(u, a.lo), a.hi);
}
__device__ __forceinline__ bool tol_has_level(const TolArgs& a, int l) { return (unsigned)l < (unsigned)a.L; }

constexpr int TOL_KT = 16;  // realisations per LDS tile
static_assert(TOL_KT * THZ_MAX_LUT == LANE_THREADS, "one level draw per thread of a tile");

template <bool WIDE>
__global__ void __launch_bounds__(LANE_THREADS) tolerance_fwd_kernel(const float2* __restrict__ f,
                                                                    const float* __restrict__ h,
                                                                    const int* __restrict__ idx,
                                                                    float2* __restrict__ out,
                                                                    float* __restrict__ hout, TolArgs a) {
  __shared__ float s_g[TOL_KT];
  __shared__ float s_e[TOL_KT][THZ_MAX_LUT];
  const long long HW = (long long)a.H * a.W;
  const int ktiles = (a.K + TOL_KT - 1) / TOL_KT;
  for (int kt = blockIdx.y; kt < ktiles; kt += gridDim.y) {
    const int j0 = kt * TOL_KT, nk = min(TOL_KT, a.K - j0);
    __syncthreads();  // the previous tile has been read
    {
      const int kk = threadIdx.x / THZ_MAX_LUT, l = threadIdx.x % THZ_MAX_LUT;
      if (kk < nk) {
        const long long k = a.first + j0 + kk;
        s_e[kk][l] = tol_level(a, k, l);
        if (l == 0) s_g[kk] = tol_scale(a, k);
      }
    }
    __syncthreads();
    for (long long c0 = (long long)blockIdx.x * LANE_CHUNK; c0 < HW; c0 += (long long)gridDim.x * LANE_CHUNK) {
      const Lane4<WIDE> Ln(c0, HW);
      float hv[LANE_PX];
      int lv[LANE_PX], sp[LANE_PX];
#pragma unroll
      for (int j = 0; j < LANE_PX; ++j) {
        const long long q = Ln.at(j);
        sp[j] = 0;
        lv[j] = -1;
        if (q < HW) {
          const int y = (int)(q / a.W), x = (int)(q - (long long)y * a.W);
          sp[j] = doe_nearest_src(y, a.hs, a.H) * a.ws + doe_nearest_src(x, a.ws, a.W);
        }
      }
      if (a.same) {
        Ln.load(h, hv);
        if (idx) Ln.load(idx, lv);
      } else {
#pragma unroll
        for (int j = 0; j < LANE_PX; ++j) {
          const bool live = Ln.at(j) < HW;
          hv[j] = live ? h[sp[j]] : 0.0f;
          if (idx && live) lv[j] = idx[sp[j]];
        }
      }
      for (int kk = 0; kk < nk; ++kk) {
        const long long k = a.first + j0 + kk;
        const float g = s_g[kk];
        float hk[LANE_PX];
#pragma unroll
        for (int j = 0; j < LANE_PX; ++j) {
          hk[j] = 0.0f;
          if (Ln.at(j) < HW) {
            const float e = tol_has_level(a, lv[j]) ? s_e[kk][lv[j]] : 0.0f;
            hk[j] = tol_height(a, hv[j], g, e, tol_rough(a, k, sp[j]), nullptr);
          }
        }
        if (hout && a.same) Ln.store(hout + (size_t)(j0 + kk) * HW, hk);
        const size_t b = a.Bf == 1 ? 0 : (size_t)(j0 + kk);
        for (int c = 0; c < a.C; ++c) {
          float2 v[LANE_PX];
          Ln.load(f + (b * a.C + c) * HW, v);
#pragma unroll
          for (int j = 0; j < LANE_PX; ++j)
            if (Ln.at(j) < HW) v[j] = cmul(v[j], doe_transmission(hk[j], a.lam[c], a.eps, a.tand, nullptr));
          Ln.store(out + ((size_t)(j0 + kk) * a.C + c) * HW, v);
        }
      }
    }
  }
}

// heights_out of a map that is not the field's size: one thread per (k, p)
__global__ void __launch_bounds__(LANE_THREADS) tolerance_heights_kernel(const float* __restrict__ h,
                                                                        const int* __restrict__ idx,
                                                                        float* __restrict__ hout, TolArgs a) {
  const long long n = (long long)a.hs * a.ws, total = n * a.K;
  for (long long i = (long long)blockIdx.x * LANE_THREADS + threadIdx.x; i < total;
       i += (long long)gridDim.x * LANE_THREADS) {
    const long long j = i / n;
    const int p = (int)(i - j * n);
    const long long k = a.first + j;
    const int l = idx ? idx[p] : -1;
    const float e = tol_has_level(a, l) ? tol_level(a, k, l) : 0.0f;
    hout[i] = tol_height(a, h[p], tol_scale(a, k), e, tol_rough(a, k, p), nullptr);
  }
}

// [*d0, *d1): the destinations dst of the nearest upsampling with doe_nearest_src(dst) == s.  The
// source index does not decrease with dst, so both ends are found by bisection on the function itself.
__device__ __forceinline__ void tol_dest_range(int s, int in, int out, int* d0, int* d1) {
  if (in == out) {
    *d0 = s;
    *d1 = s + 1;
    return;
  }
  int lo = 0, hi = out;
  while (lo < hi) {  // first dst with src >= s
    const int mid = (lo + hi) >> 1;
    if (doe_nearest_src(mid, in, out) < s) lo = mid + 1;
    else hi = mid;
  }
  *d0 = lo;
  hi = out;
  while (lo < hi) {  // first dst with src > s
    const int mid = (lo + hi) >> 1;
    if (doe_nearest_src(mid, in, out) <= s) lo = mid + 1;
    else hi = mid;
  }
  *d1 = lo;
}

constexpr int TOL_BWD_THREADS = 256;

__global__ void __launch_bounds__(TOL_BWD_THREADS) tolerance_bwd_kernel(const float2* __restrict__ G,
                                                                       const float2* __restrict__ f,
                                                                       const float* __restrict__ h,
                                                                       const int* __restrict__ idx,
                                                                       float2* __restrict__ gf,
                                                                       float* __restrict__ gh, TolArgs a) {
  const long long n = (long long)a.hs * a.ws;
  const size_t HW = (size_t)a.H * a.W;
  for (long long pp = (long long)blockIdx.x * TOL_BWD_THREADS + threadIdx.x; pp < n;
       pp += (long long)gridDim.x * TOL_BWD_THREADS) {
    const int p = (int)pp;
    const int py = p / a.ws, px = p - py * a.ws;
    int y0, y1, x0, x1;
    tol_dest_range(py, a.hs, a.H, &y0, &y1);
    tol_dest_range(px, a.ws, a.W, &x0, &x1);
    const float hv = h[p];
    const int l = idx ? idx[p] : -1;
    const bool lev = tol_has_level(a, l);
    double acc = 0.0;
    for (int c = 0; c < a.C; ++c) {
      const float lam = a.lam[c];
      for (int y = y0; y < y1; ++y) {
        for (int x = x0; x < x1; ++x) {
          const size_t q = (size_t)y * a.W + x;
          double sx = 0.0, sy = 0.0;  // sum_k G conj(t) of a one-item field
          for (int j = 0; j < a.K; ++j) {
            const long long k = a.first + j;
            const float g = tol_scale(a, k);
            const float e = lev ? tol_level(a, k, l) : 0.0f;
            bool inside;
            const float hk = tol_height(a, hv, g, e, tol_rough(a, k, p), &inside);
            float2 gam;
            const float2 t = doe_transmission(hk, lam, a.eps, a.tand, &gam);
            const float2 gv = G[((size_t)j * a.C + c) * HW + q];
            const size_t fi = ((a.Bf == 1 ? 0 : (size_t)j) * a.C + c) * HW + q;
            if (gf) {
              if (a.Bf == 1) {
                sx += (double)gv.x * t.x + (double)gv.y * t.y;
                sy += (double)gv.y * t.x - (double)gv.x * t.y;
              } else {  // thz_doe_modulate_backward's product
                gf[fi] = make_float2(gv.x * t.x + gv.y * t.y, gv.y * t.x - gv.x * t.y);
              }
            }
            if (gh && inside) {
              const float2 fv = f[fi];
              const double wr = (double)gv.x * fv.x + (double)gv.y * fv.y;  // conj(G) f
              const double wi = (double)gv.x * fv.y - (double)gv.y * fv.x;
              const double dr = (double)t.x * gam.x - (double)t.y * gam.y;  // dt/dh = t gamma
              const double di = (double)t.x * gam.y + (double)t.y * gam.x;
              acc += (double)(1.0f + g) * (wr * dr - wi * di);
            }
          }
          if (gf && a.Bf == 1) gf[(size_t)c * HW + q] = make_float2((float)sx, (float)sy);
        }
      }
    }
    if (gh) gh[p] = (float)acc;
  }
}

// ---- host side ---------------------------------------------------------------------------------
constexpr long long TOL_INDEX_RANGE = 1LL << 32;  // the generator's element index is 32-bit

// the descriptor, checked without touching the device; wavelengths are copied by the caller afterwards
static int tol_args(const char* who, const thz_tolerance_desc* d, const int* idx, TolArgs* a) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (!d->wavelengths || !d->rng) return fail(THZ_E_ARG, "%s: null wavelengths or rng", who);
  if (d->K < 1 || d->C < 1 || d->H < 1 || d->W < 1 || d->hs < 1 || d->ws < 1)
    return fail(THZ_E_ARG, "%s: bad shape K=%d C=%d field %dx%d map %dx%d", who, d->K, d->C, d->H, d->W, d->hs, d->ws);
  if (d->Bf != 1 && d->Bf != d->K) return fail(THZ_E_ARG, "%s: the field has Bf = %d items, not 1 or K = %d", who, d->Bf, d->K);
  if (d->C > THZ_MAX_WAVELENGTHS) return fail(THZ_E_UNSUPPORTED, "%s: C=%d > %d", who, d->C, THZ_MAX_WAVELENGTHS);
  if ((long long)d->H * d->W > INT_MAX || (long long)d->hs * d->ws > INT_MAX)
    return fail(THZ_E_UNSUPPORTED, "%s: a plane of more than 2^31 - 1 pixels", who);
  if (d->L < 0 || d->L > THZ_MAX_LUT) return fail(THZ_E_ARG, "%s: L = %d outside [0, %d]", who, d->L, THZ_MAX_LUT);
  if (!(d->sigma_scale >= 0.0f)) return fail(THZ_E_ARG, "%s: sigma_scale = %g < 0", who, (double)d->sigma_scale);
  bool level_term = false;
  for (int l = 0; l < d->L; ++l) {
    if (!(d->sigma_level[l] >= 0.0f)) return fail(THZ_E_ARG, "%s: sigma_level[%d] = %g < 0", who, l, (double)d->sigma_level[l]);
    level_term = level_term || d->sigma_level[l] != 0.0f;
  }
  if (d->rough_kind < THZ_TOL_ROUGH_NONE || d->rough_kind > THZ_TOL_ROUGH_NORMAL)
    return fail(THZ_E_ARG, "%s: roughness kind %d", who, d->rough_kind);
  if (!(d->rough >= 0.0f)) return fail(THZ_E_ARG, "%s: roughness = %g < 0", who, (double)d->rough);
  if (!(d->lo <= d->hi)) return fail(THZ_E_ARG, "%s: clamp lo = %g > hi = %g", who, (double)d->lo, (double)d->hi);
  if (d->first < 0) return fail(THZ_E_ARG, "%s: first = %lld < 0", who, d->first);
  const long long n = (long long)d->hs * d->ws;
  if (d->first > TOL_INDEX_RANGE || d->first + d->K > TOL_INDEX_RANGE / 16)
    return fail(THZ_E_ARG, "%s: (first + K) 16 = (%lld + %d) 16 > 2^32, the generator's index range", who, d->first, d->K);
  if (d->first + d->K > TOL_INDEX_RANGE / n)
    return fail(THZ_E_ARG, "%s: (first + K) hs ws = (%lld + %d) %lld > 2^32, the generator's index range", who,
                d->first, d->K, n);
  if (level_term && !idx) return fail(THZ_E_ARG, "%s: null idx with a non-zero sigma_level", who);
  if (int e = check_arrays(who, {d->rng}, sizeof(unsigned))) return e;
  if (idx && misaligned(idx, sizeof(int))) return fail(THZ_E_ARG, "%s: array not 4-byte aligned", who);
  a->K = d->K; a->Bf = d->Bf; a->C = d->C; a->H = d->H; a->W = d->W; a->hs = d->hs; a->ws = d->ws;
  a->L = d->L;
  a->rough_kind = d->rough_kind;
  a->same = d->hs == d->H && d->ws == d->W;
  a->first = d->first;
  a->sigma_scale = d->sigma_scale; a->rough = d->rough; a->lo = d->lo; a->hi = d->hi;
  a->eps = d->epsilon; a->tand = d->tand;
  a->rng = d->rng;
  a->stream = d->stream;
  for (int l = 0; l < THZ_MAX_LUT; ++l) a->sigma_level[l] = l < d->L ? d->sigma_level[l] : 0.0f;
  return THZ_OK;
}

}  // namespace thz

using namespace thz;

extern "C" int thz_tolerance_modulate_forward(const thz_tolerance_desc* d, const void* field, const float* height,
                                              const int* idx, void* out, float* heights_out, thz_stream_t stream) {
  const char* who = "thz_tolerance_modulate_forward";
  TolArgs a{};
  if (int e = tol_args(who, d, idx, &a)) return e;
  if (int e = check_arrays(who, {field, out}, sizeof(float2))) return e;
  if (int e = check_arrays(who, {height}, sizeof(float))) return e;
  if (heights_out && misaligned(heights_out, sizeof(float))) return fail(THZ_E_ARG, "%s: array not 4-byte aligned", who);
  for (int c = 0; c < d->C; ++c) a.lam[c] = d->wavelengths[c];
  hipStream_t s = (hipStream_t)stream;
  const long long HW = (long long)d->H * d->W;
  const long long chunks = (HW + LANE_CHUNK - 1) / LANE_CHUNK, ktiles = (d->K + TOL_KT - 1) / TOL_KT;
  int blocks = 0;
  if (int e = stream_grid(chunks * ktiles, &blocks)) return e;
  const long long gx = chunks < blocks ? chunks : blocks;
  const long long gy = ktiles < blocks / gx ? ktiles : (blocks / gx > 1 ? blocks / gx : 1);
  const dim3 grid((unsigned)gx, (unsigned)gy);
  const bool wide = HW % LANE_PX == 0 && all_aligned16({field, out, a.same ? (const void*)height : nullptr,
                                                        a.same ? (const void*)idx : nullptr,
                                                        a.same ? (const void*)heights_out : nullptr});
  KernelTimer kt("tolerance_fwd", s);
  if (wide)
    hipLaunchKernelGGL(tolerance_fwd_kernel<true>, grid, dim3(LANE_THREADS), 0, s, (const float2*)field, height, idx,
                       (float2*)out, heights_out, a);
  else
    hipLaunchKernelGGL(tolerance_fwd_kernel<false>, grid, dim3(LANE_THREADS), 0, s, (const float2*)field, height, idx,
                       (float2*)out, heights_out, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  if (heights_out && !a.same) {
    const long long total = (long long)d->hs * d->ws * d->K;
    if (int e = stream_grid((total + LANE_THREADS - 1) / LANE_THREADS, &blocks)) return e;
    KernelTimer kh("tolerance_heights", s);
    hipLaunchKernelGGL(tolerance_heights_kernel, dim3((unsigned)blocks), dim3(LANE_THREADS), 0, s, height, idx,
                       heights_out, a);
    THZ_LAUNCH_CHECK();
    kh.stop();
  }
  return THZ_OK;
}

extern "C" int thz_tolerance_modulate_backward(const thz_tolerance_desc* d, const void* grad_out, const void* field,
                                               const float* height, const int* idx, void* grad_field,
                                               float* grad_height, void* workspace, size_t bytes,
                                               thz_stream_t stream) {
  const char* who = "thz_tolerance_modulate_backward";
  (void)workspace;  // reserved: the backward needs none
  (void)bytes;
  TolArgs a{};
  if (int e = tol_args(who, d, idx, &a)) return e;
  if (int e = check_arrays(who, {grad_out, field}, sizeof(float2))) return e;
  if (int e = check_arrays(who, {height}, sizeof(float))) return e;
  if (grad_field && misaligned(grad_field, sizeof(float2))) return fail(THZ_E_ARG, "%s: array not 8-byte aligned", who);
  if (grad_height && misaligned(grad_height, sizeof(float))) return fail(THZ_E_ARG, "%s: array not 4-byte aligned", who);
  if (!grad_field && !grad_height) return THZ_OK;  // nothing asked for
  for (int c = 0; c < d->C; ++c) a.lam[c] = d->wavelengths[c];
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)d->hs * d->ws;
  int blocks = 0;
  if (int e = stream_grid((n + TOL_BWD_THREADS - 1) / TOL_BWD_THREADS, &blocks)) return e;
  // a map with more pixels than the field leaves field pixels' owners in place but map pixels without
  // readers: their gradient is the empty sum, written as 0 by the owning thread
  KernelTimer kt("tolerance_bwd", s);
  hipLaunchKernelGGL(tolerance_bwd_kernel, dim3((unsigned)blocks), dim3(TOL_BWD_THREADS), 0, s, (const float2*)grad_out,
                     (const float2*)field, height, idx, (float2*)grad_field, grad_height, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
