// Height-map helpers: the look-up-table quantizers with surrogate gradients (utils/Helper_Functions.py:375-398,
// Components/quantization.py:59-127, the notebooks' argmin snap) and the total-variation regulariser
// (utils/Helper_Functions.py:40-70) as fused kernels.
//
//   thz_lut_quantize_forward   one streaming pass: q = lut[idx], idx by counting thresholds (bucketize) or
//                              by the first minimum of |x - lut[j]| (argmin).  The thresholds / levels are
//                              wave-uniform operands read from the kernel arguments; a lane's divergent
//                              lut[idx] reads a copy of the table in LDS.
//   thz_lut_quantize_backward  one streaming pass: grad_out times the identity / polynomial / sigmoid
//                              surrogate slope, s from device memory.
//   thz_tv_forward             center_difference or the two L1 sums of it.  A wave owns a 256-column x
//                              32-row tile, a lane four consecutive columns; the lane walks down the rows
//                              holding rows i - 1, i, i + 1 in registers and takes the columns beside
//                              its four from the neighbouring lanes, so x is read once plus the tile's
//                              halo (2 of 34 rows, 2 of 258 columns).  Chosen over an LDS tile: the
//                              stencil reuses a value three times along each axis, which registers and
//                              one cross-lane move serve without a barrier or an LDS round trip.
//   thz_tv_backward            the adjoint stencil gathered per element on the same tiles (window of
//                              five rows and two columns each side for total_variation, whose
//                              cotangent sign(dx), sign(dy) is recomputed from x).
// fp32 throughout, contraction off: a result does not depend on which form (16-byte or element
// width) moved it, and the quantizer's comparisons are the ones torch makes.
#include <cstdint>
#include <initializer_list>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_stream.hpp"
#include "thz_launch.hpp"

namespace thz {

#pragma clang fp contract(off)

// ---- LUT quantizers --------------------------------------------------------------------------
struct LutArgs {
  int L, T, wrap;
  float lut[THZ_MAX_LUT];
  float thr[THZ_MAX_LUT];
};

// the table in LDS for a lane's own (divergent) index
__device__ __forceinline__ void lut_to_lds(const LutArgs& a, float* s_lut) {
#pragma unroll
  for (int j = 0; j < THZ_MAX_LUT; ++j)
    if (threadIdx.x == j) s_lut[j] = a.lut[j];  // lut_args zero-fills past L
  __syncthreads();
}

template <int MODE, bool WIDE>
__global__ void __launch_bounds__(LANE_THREADS) lut_quantize_fwd_kernel(LutArgs a, const float* __restrict__ x,
                                                                       long long n, float* __restrict__ q,
                                                                       int* __restrict__ idx) {
  __shared__ float s_lut[THZ_MAX_LUT];
  lut_to_lds(a, s_lut);
  for (long long c0 = (long long)blockIdx.x * LANE_CHUNK; c0 < n; c0 += (long long)gridDim.x * LANE_CHUNK) {
    const Lane4<WIDE> lane(c0, n);
    float v[LANE_PX], qo[LANE_PX];
    int io[LANE_PX];
    lane.load(x, v);
    if (MODE == THZ_LUTQ_BUCKETIZE) {
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k) io[k] = 0;
      for (int j = 0; j < a.T; ++j) {  // wave-uniform j: the threshold is a scalar operand
        const float t = a.thr[j];
#pragma unroll
        for (int k = 0; k < LANE_PX; ++k) io[k] += !(t > v[k]);  // upper bound; NaN counts every threshold
      }
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k) {
        if (a.wrap && io[k] == a.T) io[k] = 0;  // io <= T, so this is io mod T
        qo[k] = s_lut[io[k]];  // io < L by the host's check of T
      }
    } else {
      float best[LANE_PX];
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k) {
        io[k] = 0;
        qo[k] = a.lut[0];
        best[k] = fabsf(v[k] - qo[k]);
      }
      for (int j = 1; j < a.L; ++j) {
        const float l = a.lut[j];
#pragma unroll
        for (int k = 0; k < LANE_PX; ++k) {
          const float dj = fabsf(v[k] - l);
          if (dj < best[k]) {  // strict: ties keep the lower index; NaN never wins
            best[k] = dj;
            io[k] = j;
            qo[k] = l;
          }
        }
      }
    }
    lane.store(q, qo);
    lane.store(idx, io);
  }
}

// torch.nan_to_num at its defaults
__device__ __forceinline__ float nan_to_num(float v) {
  if (v != v) return 0.0f;
  return fminf(fmaxf(v, -3.402823466e+38f), 3.402823466e+38f);
}

// the surrogate slope in the reference's op order (Components/quantization.py:83-94, :108-120)
template <int KIND>
__device__ __forceinline__ float lut_slope(float x, int i, float s, int L, const float* s_lut) {
  if (KIND == THZ_LUTQ_GRAD_IDENTITY) return 1.0f;
  i = i < 0 ? 0 : i >= L ? L - 1 : i;
  const float q = s_lut[i];
  const float dx = x - q;
  const int d = fabsf(dx) < __builtin_inff() ? (dx > 0.0f) - (dx < 0.0f) : 0;
  int j = i + d;
  j = j < 0 ? L - 1 : j >= L ? 0 : j;
  const float other = s_lut[j];
  const float mid = (other + q) / 2.0f;
  const float gap = fabsf(other - q) + 1e-20f;
  float z = (x - mid) / gap * 2.0f;
  if (KIND == THZ_LUTQ_GRAD_POLY) return nan_to_num(0.5f * s * powf(1.0f - fabsf(z), s - 1.0f)) * 2.0f;
  z *= s;
  const float sg = 1.0f / (1.0f + expf(-z));
  return sg * (1.0f - sg) * (4.0f * s);
}

template <int KIND, bool WIDE>
__global__ void __launch_bounds__(LANE_THREADS) lut_quantize_bwd_kernel(LutArgs a, const float* __restrict__ x,
                                                                       const int* __restrict__ idx,
                                                                       const float* __restrict__ g,
                                                                       const float* __restrict__ s_dev, long long n,
                                                                       float* __restrict__ out) {
  __shared__ float s_lut[THZ_MAX_LUT];
  lut_to_lds(a, s_lut);
  const float s = KIND == THZ_LUTQ_GRAD_IDENTITY ? 1.0f : *s_dev;
  for (long long c0 = (long long)blockIdx.x * LANE_CHUNK; c0 < n; c0 += (long long)gridDim.x * LANE_CHUNK) {
    const Lane4<WIDE> lane(c0, n);
    float v[LANE_PX], gv[LANE_PX], o[LANE_PX];
    int iv[LANE_PX];
    lane.load(g, gv);
    if (KIND != THZ_LUTQ_GRAD_IDENTITY) {
      lane.load(x, v);
      lane.load(idx, iv);
    }
#pragma unroll
    for (int k = 0; k < LANE_PX; ++k) o[k] = gv[k] * lut_slope<KIND>(v[k], iv[k], s, a.L, s_lut);
    lane.store(out, o);
  }
}

// ---- total variation -------------------------------------------------------------------------
constexpr int TV_COLS = 64 * LANE_PX;  // a wave's tile: 256 columns (four per lane) ...
constexpr int TV_ROWS = 32;           // ... by 32 rows
constexpr int TV_WAVES = LANE_THREADS / 64;
constexpr int TV_MAX_EDGE = 1 << 30;  // rows / columns: a tile's end (edge + tile size) stays an int

struct TvShape {
  long long N;
  int H, W;
  int tx, ty;       // tiles across and down a plane
  long long tiles;  // N ty tx
  bool wide;        // rows start 16-byte aligned: W % 4 == 0 and every base pointer aligned
};

// a wave's tile and its lane's four columns
struct TvTile {
  long long plane;  // element offset of the plane
  int r0, r1, c0;   // rows [r0, r1), the lane's columns c0 .. c0 + 3
  bool valid;
  __device__ __forceinline__ TvTile(const TvShape& s) {
    const long long t = (long long)blockIdx.x * TV_WAVES + (threadIdx.x >> 6);
    valid = t < s.tiles;
    const long long per = (long long)s.tx * s.ty, n = valid ? t / per : 0;
    const long long rem = valid ? t - n * per : 0;  // < tx ty, which can pass the int range
    plane = n * s.H * s.W;
    r0 = (int)(rem / s.tx) * TV_ROWS;  // < H + TV_ROWS and c0 < W + TV_COLS: ints by tv_shape's bound on H, W
    r1 = r0 + TV_ROWS < s.H ? r0 + TV_ROWS : s.H;
    c0 = (int)(rem % s.tx) * TV_COLS + (threadIdx.x & 63) * LANE_PX;
  }
};

// the lane's four values of row i, zero outside the plane (a row outside it has no columns)
__device__ __forceinline__ void tv_row(const float* __restrict__ p, const TvShape& s, const TvTile& t, int i,
                                       float v[LANE_PX]) {
  const bool in = i >= 0 && i < s.H;
  ld4(p + t.plane + (long long)(in ? i : 0) * s.W, t.c0, in ? s.W : 0, s.wide, v);
}
__device__ __forceinline__ void tv_store(float* __restrict__ p, const TvShape& s, const TvTile& t, int i,
                                         const float v[LANE_PX]) {
  st4(p + t.plane + (long long)i * s.W, t.c0, s.W, s.wide, v);
}

// xx[0 .. 2 D + 3] = row i at columns c0 - D .. c0 + 3 + D: the lane's own four (v), the D beside them from
// the neighbouring lanes, and at the wave's first / last lane from memory (zero outside the plane).
// Every lane of the wave calls it.
template <int D>
__device__ __forceinline__ void tv_span(const float* __restrict__ p, const TvShape& s, const TvTile& t, int i,
                                        const float v[LANE_PX], float xx[LANE_PX + 2 * D]) {
  const int lane = threadIdx.x & 63;
  const bool in = i >= 0 && i < s.H;
  const float* row = p + t.plane + (long long)(in ? i : 0) * s.W;
#pragma unroll
  for (int k = 0; k < LANE_PX; ++k) xx[D + k] = v[k];
#pragma unroll
  for (int e = 1; e <= D; ++e) {
    float l = __shfl_up(v[LANE_PX - e], 1), r = __shfl_down(v[e - 1], 1);
    const int cl = t.c0 - e, cr = t.c0 + LANE_PX - 1 + e;
    if (lane == 0) l = in && cl >= 0 && cl < s.W ? row[cl] : 0.0f;
    if (lane == 63) r = in && cr < s.W ? row[cr] : 0.0f;
    xx[D - e] = l;
    xx[D + LANE_PX - 1 + e] = r;
  }
}

// -a + 2 b - c as torch evaluates W / 4 * (-x[j-1] + 2 x[j] - x[j+1]) before the scale
__device__ __forceinline__ float tv_stencil(float a, float b, float c) { return (-a + 2.0f * b) - c; }
__device__ __forceinline__ float tv_sign(float v) { return (float)((v > 0.0f) - (v < 0.0f)); }

// SUMS: partial[2 block + {0, 1}] = the workgroup's sum |dx|, sum |dy|; else dx, dy are written
template <bool SUMS>
__global__ void __launch_bounds__(LANE_THREADS) tv_fwd_kernel(TvShape s, const float* __restrict__ x,
                                                             float* __restrict__ dx, float* __restrict__ dy,
                                                             double* __restrict__ partial) {
  const TvTile t(s);
  const float cw = (float)((double)s.W / 4.0), ch = (float)((double)s.H / 4.0);
  double sx = 0.0, sy = 0.0;
  if (t.valid) {  // wave-uniform
    float up[LANE_PX], cur[LANE_PX], dn[LANE_PX];
    tv_row(x, s, t, t.r0 - 1, up);
    tv_row(x, s, t, t.r0, cur);
    for (int i = t.r0; i < t.r1; ++i) {
      tv_row(x, s, t, i + 1, dn);
      float xx[LANE_PX + 2], ox[LANE_PX], oy[LANE_PX];
      tv_span<1>(x, s, t, i, cur, xx);
      const bool row_in = i >= 1 && i <= s.H - 2;
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k) {
        const int c = t.c0 + k;
        ox[k] = c >= 1 && c <= s.W - 2 ? cw * tv_stencil(xx[k], xx[k + 1], xx[k + 2]) : 0.0f;
        oy[k] = row_in && c < s.W ? ch * tv_stencil(up[k], cur[k], dn[k]) : 0.0f;
        if (SUMS) {
          sx += (double)fabsf(ox[k]);
          sy += (double)fabsf(oy[k]);
        }
        up[k] = cur[k];
        cur[k] = dn[k];
      }
      if (!SUMS) {
        tv_store(dx, s, t, i, ox);
        tv_store(dy, s, t, i, oy);
      }
    }
  }
  if (SUMS) store_partials(Sums<2>{{sx, sy}}, partial, blockIdx.x);
}

// tv = sum |dx| / count + sum |dy| / count, the partials added in index order
__global__ void __launch_bounds__(LANE_THREADS) tv_finish_kernel(const double* __restrict__ partial, long long blocks,
                                                                double count, float* __restrict__ tv) {
  const Sums<2> a = gather_partials<2>(partial, blocks);
  if (threadIdx.x == 0) *tv = (float)(a.v[0] / count + a.v[1] / count);
}

// FROM_X: u, v = sign(dx), sign(dy) recomputed from x (a), scaled by *grad_loss / (N H W);
// else u = a (the cotangent of dx), v = b (the cotangent of dy)
template <bool FROM_X>
__global__ void __launch_bounds__(LANE_THREADS) tv_bwd_kernel(TvShape s, const float* __restrict__ a,
                                                             const float* __restrict__ b,
                                                             const float* __restrict__ grad_loss,
                                                             float* __restrict__ grad) {
  constexpr int D = FROM_X ? 2 : 1;  // rows / columns needed beside an element
  const TvTile t(s);
  if (!t.valid) return;  // wave-uniform; no barrier below
  const float* vsrc = FROM_X ? a : b;
  const double cnt = FROM_X ? (double)s.N * (double)s.H * (double)s.W : 1.0;
  const float cw = (float)((double)s.W / (4.0 * cnt)), ch = (float)((double)s.H / (4.0 * cnt));
  const float gl = FROM_X ? *grad_loss : 1.0f;
  float win[2 * D + 1][LANE_PX];  // rows i - D .. i + D of vsrc
#pragma unroll
  for (int r = 1; r <= 2 * D; ++r) tv_row(vsrc, s, t, t.r0 - D + r - 1, win[r]);
  for (int i = t.r0; i < t.r1; ++i) {
#pragma unroll
    for (int r = 0; r < 2 * D; ++r)
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k) win[r][k] = win[r + 1][k];
    tv_row(vsrc, s, t, i + D, win[2 * D]);
    float hrow[LANE_PX], xx[LANE_PX + 2 * D], u[LANE_PX + 2], o[LANE_PX];
    if constexpr (FROM_X) {
#pragma unroll
      for (int k = 0; k < LANE_PX; ++k) hrow[k] = win[D][k];
    } else {
      tv_row(a, s, t, i, hrow);
    }
    tv_span<D>(a, s, t, i, hrow, xx);
    // u at columns c0 - 1 .. c0 + 4, zero outside the interior columns
#pragma unroll
    for (int k = 0; k < LANE_PX + 2; ++k) {
      const int c = t.c0 - 1 + k;
      float val;
      if constexpr (FROM_X) val = tv_sign(tv_stencil(xx[k], xx[k + 1], xx[k + 2]));
      else val = xx[k];
      u[k] = c >= 1 && c <= s.W - 2 ? val : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < LANE_PX; ++k) {
      float v[3];  // rows i - 1, i, i + 1, zero outside the interior rows
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int row = i - 1 + r;
        float val;
        if constexpr (FROM_X) val = tv_sign(tv_stencil(win[r][k], win[r + 1][k], win[r + 2][k]));
        else val = win[r][k];
        v[r] = row >= 1 && row <= s.H - 2 ? val : 0.0f;
      }
      const float ix = (2.0f * u[k + 1] - u[k]) - u[k + 2], iy = (2.0f * v[1] - v[0]) - v[2];
      o[k] = gl * (cw * ix + ch * iy);
    }
    tv_store(grad, s, t, i, o);
  }
}

#pragma clang fp contract(on)

// ---- host side -------------------------------------------------------------------------------
// every array of this unit is float32 or int32
static int check_ptrs(const char* who, std::initializer_list<const void*> ptrs) { return check_arrays(who, ptrs, 4); }

static int lut_check(const char* who, const thz_lut_quantize_desc* d, bool forward) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->n < 0) return fail(THZ_E_ARG, "%s: n = %lld < 0", who, d->n);
  if (d->L < 1 || d->L > THZ_MAX_LUT)
    return fail(THZ_E_UNSUPPORTED, "%s: %d levels (1 .. %d)", who, d->L, THZ_MAX_LUT);
  if (forward) {
    if (d->mode != THZ_LUTQ_BUCKETIZE && d->mode != THZ_LUTQ_ARGMIN) return fail(THZ_E_ARG, "%s: mode %d", who, d->mode);
    if (d->mode == THZ_LUTQ_BUCKETIZE) {
      const int lo = d->wrap ? 1 : 0, hi = d->wrap ? d->L : d->L - 1;
      if (d->T < lo || d->T > hi)
        return fail(THZ_E_ARG, "%s: %d thresholds for %d levels (%d .. %d%s)", who, d->T, d->L, lo, hi,
                    d->wrap ? ", wrap" : "");
    }
  } else if (d->kind < THZ_LUTQ_GRAD_IDENTITY || d->kind > THZ_LUTQ_GRAD_SIGMOID) {
    return fail(THZ_E_ARG, "%s: kind %d", who, d->kind);
  }
  return THZ_OK;
}

static LutArgs lut_args(const thz_lut_quantize_desc* d) {
  LutArgs a{};
  a.L = d->L;
  a.T = d->mode == THZ_LUTQ_BUCKETIZE ? d->T : 0;
  a.wrap = d->wrap != 0;
  for (int k = 0; k < THZ_MAX_LUT; ++k) {
    a.lut[k] = k < d->L ? d->lut[k] : 0.0f;
    a.thr[k] = k < a.T ? d->thresholds[k] : 0.0f;
  }
  return a;
}

static int tv_shape(const char* who, long long N, int H, int W, TvShape* s) {
  if (N < 1 || H < 1 || W < 1) return fail(THZ_E_ARG, "%s: bad shape N = %lld, H = %d, W = %d", who, N, H, W);
  if (H > TV_MAX_EDGE || W > TV_MAX_EDGE)
    return fail(THZ_E_UNSUPPORTED, "%s: H = %d, W = %d beyond 2^30 rows / columns", who, H, W);
  s->N = N;
  s->H = H;
  s->W = W;
  s->tx = (W + TV_COLS - 1) / TV_COLS;
  s->ty = (H + TV_ROWS - 1) / TV_ROWS;
  if (N > (((1LL << 31) - 1) * TV_WAVES) / ((long long)s->tx * s->ty))
    return fail(THZ_E_UNSUPPORTED, "%s: N = %lld planes of %d x %d beyond the grid's extent", who, N, H, W);
  s->tiles = N * s->tx * s->ty;
  s->wide = false;
  return THZ_OK;
}
static long long tv_blocks(const TvShape& s) { return (s.tiles + TV_WAVES - 1) / TV_WAVES; }
static size_t tv_workspace(const TvShape& s) { return align256(sizeof(double) * 2 * (size_t)tv_blocks(s)); }

}  // namespace thz

using namespace thz;

extern "C" int thz_lut_quantize_forward(const thz_lut_quantize_desc* d, const float* x, float* q, int* idx,
                                        thz_stream_t stream) {
  const char* who = "thz_lut_quantize_forward";
  if (int e = lut_check(who, d, true)) return e;
  if (int e = check_ptrs(who, {x, q, idx})) return e;
  if (d->n == 0) return THZ_OK;
  hipStream_t s = (hipStream_t)stream;
  int blocks = 0;
  if (int e = stream_grid((d->n + LANE_CHUNK - 1) / LANE_CHUNK, &blocks)) return e;
  const LutArgs a = lut_args(d);
  const bool wide = all_aligned16({x, q, idx});
  const dim3 g((unsigned)blocks), b(LANE_THREADS);
  KernelTimer kt("lut_quantize_fwd", s);
  auto launch = [&](auto MODE) {
    if (wide) hipLaunchKernelGGL((lut_quantize_fwd_kernel<MODE(), true>), g, b, 0, s, a, x, d->n, q, idx);
    else hipLaunchKernelGGL((lut_quantize_fwd_kernel<MODE(), false>), g, b, 0, s, a, x, d->n, q, idx);
  };
  if (d->mode == THZ_LUTQ_BUCKETIZE) launch(Size<THZ_LUTQ_BUCKETIZE>{});
  else launch(Size<THZ_LUTQ_ARGMIN>{});
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_lut_quantize_backward(const thz_lut_quantize_desc* d, const float* x, const int* idx,
                                         const float* grad_out, const float* s_dev, float* grad_in,
                                         thz_stream_t stream) {
  const char* who = "thz_lut_quantize_backward";
  if (int e = lut_check(who, d, false)) return e;
  if (int e = check_ptrs(who, {grad_out, grad_in})) return e;
  const bool identity = d->kind == THZ_LUTQ_GRAD_IDENTITY;
  if (!identity)
    if (int e = check_ptrs(who, {x, idx, s_dev})) return e;
  if (d->n == 0) return THZ_OK;
  hipStream_t s = (hipStream_t)stream;
  int blocks = 0;
  if (int e = stream_grid((d->n + LANE_CHUNK - 1) / LANE_CHUNK, &blocks)) return e;
  const LutArgs a = lut_args(d);
  const bool wide = identity ? all_aligned16({grad_out, grad_in}) : all_aligned16({x, idx, grad_out, grad_in});
  const dim3 g((unsigned)blocks), b(LANE_THREADS);
  KernelTimer kt("lut_quantize_bwd", s);
  auto launch = [&](auto KIND) {
    if (wide)
      hipLaunchKernelGGL((lut_quantize_bwd_kernel<KIND(), true>), g, b, 0, s, a, x, idx, grad_out, s_dev, d->n, grad_in);
    else
      hipLaunchKernelGGL((lut_quantize_bwd_kernel<KIND(), false>), g, b, 0, s, a, x, idx, grad_out, s_dev, d->n, grad_in);
  };
  if (identity) launch(Size<THZ_LUTQ_GRAD_IDENTITY>{});
  else if (d->kind == THZ_LUTQ_GRAD_POLY) launch(Size<THZ_LUTQ_GRAD_POLY>{});
  else launch(Size<THZ_LUTQ_GRAD_SIGMOID>{});
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_tv_workspace_size(long long N, int H, int W, size_t* bytes) {
  const char* who = "thz_tv_workspace_size";
  if (!bytes) return fail(THZ_E_ARG, "%s: null pointer", who);
  TvShape sh;
  if (int e = tv_shape(who, N, H, W, &sh)) return e;
  *bytes = tv_workspace(sh);
  return THZ_OK;
}

extern "C" int thz_tv_forward(const float* x, long long N, int H, int W, float* dx, float* dy, float* tv,
                              void* workspace, size_t bytes, thz_stream_t stream) {
  const char* who = "thz_tv_forward";
  TvShape sh;
  if (int e = tv_shape(who, N, H, W, &sh)) return e;
  if (int e = check_ptrs(who, {x})) return e;
  if ((dx == nullptr) != (dy == nullptr)) return fail(THZ_E_ARG, "%s: dx and dy go together", who);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g((unsigned)tv_blocks(sh)), b(LANE_THREADS);
  if (dx) {
    if (int e = check_ptrs(who, {dx, dy})) return e;
    sh.wide = W % 4 == 0 && all_aligned16({x, dx, dy});
    KernelTimer kt("center_difference", s);
    hipLaunchKernelGGL(tv_fwd_kernel<false>, g, b, 0, s, sh, x, dx, dy, (double*)nullptr);
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  }
  if (int e = check_ptrs(who, {tv})) return e;
  if (workspace && misaligned(workspace, sizeof(double))) return fail(THZ_E_ARG, "%s: workspace misaligned", who);
  if (int e = check_workspace(workspace, bytes, tv_workspace(sh))) return e;
  sh.wide = W % 4 == 0 && all_aligned16({x});
  double* partial = (double*)workspace;
  KernelTimer kt("tv_fwd", s);
  hipLaunchKernelGGL(tv_fwd_kernel<true>, g, b, 0, s, sh, x, (float*)nullptr, (float*)nullptr, partial);
  THZ_LAUNCH_CHECK();
  kt.stop();
  KernelTimer kf("tv_finish", s);
  hipLaunchKernelGGL(tv_finish_kernel, dim3(1), b, 0, s, (const double*)partial, tv_blocks(sh),
                     (double)N * (double)H * (double)W, tv);
  THZ_LAUNCH_CHECK();
  kf.stop();
  return THZ_OK;
}

extern "C" int thz_tv_backward(const float* x, const float* gdx, const float* gdy, const float* grad_loss, long long N,
                               int H, int W, float* grad, thz_stream_t stream) {
  const char* who = "thz_tv_backward";
  TvShape sh;
  if (int e = tv_shape(who, N, H, W, &sh)) return e;
  if (int e = check_ptrs(who, {grad})) return e;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g((unsigned)tv_blocks(sh)), b(LANE_THREADS);
  if (x) {
    if (gdx || gdy) return fail(THZ_E_ARG, "%s: x (total_variation) or gdx, gdy (center_difference), not both", who);
    if (int e = check_ptrs(who, {x, grad_loss})) return e;
    sh.wide = W % 4 == 0 && all_aligned16({x, grad});
    KernelTimer kt("tv_bwd", s);
    hipLaunchKernelGGL(tv_bwd_kernel<true>, g, b, 0, s, sh, x, (const float*)nullptr, grad_loss, grad);
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  }
  if (int e = check_ptrs(who, {gdx, gdy})) return e;
  sh.wide = W % 4 == 0 && all_aligned16({gdx, gdy, grad});
  KernelTimer kt("center_difference_bwd", s);
  hipLaunchKernelGGL(tv_bwd_kernel<false>, g, b, 0, s, sh, gdx, gdy, (const float*)nullptr, grad);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
