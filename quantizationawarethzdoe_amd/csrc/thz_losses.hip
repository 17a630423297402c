// The image losses of utils/losses.py (BinaryDiceLoss :7-44, BinaryCEloss :47-58, SSIMloss :62-74,
// Hierarchyloss :78-88) as fused kernels.
//
//   thz_dice_bce_sums      one streaming pass over pred, target viewed as [N, M]: the four per-sample
//                          sums  sum p t, sum p^e, sum t^e, sum bce(p, t)  (and, on request, the
//                          elementwise BCE map).  fp64 partial per workgroup, then a finish kernel --
//                          the two-stage sum of thz_signal_scale (thz_noise.hip), no atomics.
//   thz_dice_bce_backward  one streaming pass: grad_pred from the saved sums and the upstream
//                          gradients (device memory), Dice and / or BCE term.
//   thz_ssim_forward       one workgroup per 32 x 32 tile of the window-position map: stages its
//                          (32 + ws - 1)^2 tiles of x and y in LDS, runs the horizontal then the
//                          vertical pass of the 1-D window over x, y, x^2, y^2, xy in fp64, forms S and
//                          cs per position, fp64 partial per workgroup; a finish kernel writes the
//                          per-plane means.  On request it also writes the backward's coefficient planes.
//   thz_ssim_backward      the adjoint separable correlation of the three coefficient planes, as a
//                          gather over a 32 x 32 tile of pixels: no atomics.
// Why fp64 inside the SSIM forward: sigma^2 = m_xx - mu^2 cancels; in fp32 the rounding of the two
// 11-tap sums is amplified by 1 / C2 = 1e3 .. 1e4 into S, and on a flat region it does not average
// out over the positions.  The inputs stay fp32 in LDS (exact), the sums are fp64 (half the fp32
// rate on this part; the kernel is bound by LDS traffic).
#include <cstdint>
#include <initializer_list>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_stream.hpp"
#include "thz_launch.hpp"

namespace thz {

// ---- Dice / BCE ------------------------------------------------------------------------------
// Contraction off: the 16-byte and the element-width form of a kernel then give the same bits per
// element (as thz_noise.hip), so a result does not depend on the alignment of the arrays.
#pragma clang fp contract(off)
struct DiceBceArgs {
  const float *pred, *target, *weight, *pos_weight;
  float* map;
  long long M;
  int parts;  // workgroups per sample
  int terms;
  float p;
};

// x^e of the Dice denominator: e = 1 and e = 2 without powf
template <int PK>
__device__ __forceinline__ float dice_pow(float v, float e) {
  return PK == 1 ? v : PK == 2 ? v * v : powf(v, e);
}
// d/dv v^e
template <int PK>
__device__ __forceinline__ float dice_dpow(float v, float e) {
  return PK == 1 ? 1.0f : PK == 2 ? 2.0f * v : e * powf(v, e - 1.0f);
}

// BCE with logits, the stable form; weighted: torch's (1 - t) x + (1 + (pw - 1) t) (log1p(exp(-|x|)) + max(-x, 0)),
// times w (utils/losses.py:54 hands weight and pos_weight to torch.nn.BCEWithLogitsLoss)
template <bool WEIGHTED>
__device__ __forceinline__ float bce_value(float x, float t, float w, float pw) {
  const float sp = log1pf(expf(-fabsf(x)));
  if (!WEIGHTED) return fmaxf(x, 0.0f) - x * t + sp;
  return ((1.0f - t) * x + (1.0f + (pw - 1.0f) * t) * (sp + fmaxf(-x, 0.0f))) * w;
}
// its derivative in x: sigma(x) - t, weighted w ((1 - t) - (1 + (pw - 1) t) (1 - sigma(x)))
template <bool WEIGHTED>
__device__ __forceinline__ float bce_slope(float x, float t, float w, float pw) {
  const float e = expf(-fabsf(x));
  const float r = 1.0f / (1.0f + e);
  const float sig = x >= 0.0f ? r : e * r, nsig = x >= 0.0f ? e * r : r;  // sigma(x), 1 - sigma(x)
  if (!WEIGHTED) return sig - t;
  return w * ((1.0f - t) - (1.0f + (pw - 1.0f) * t) * nsig);
}

__device__ __forceinline__ void fill_ones(float v[LANE_PX]) {
#pragma unroll
  for (int k = 0; k < LANE_PX; ++k) v[k] = 1.0f;
}

// partial[(n parts + part) 4 + k]: sample n's four sums over the chunks part, part + parts, ...
template <int PK, bool WEIGHTED>
__global__ void __launch_bounds__(LANE_THREADS) dice_bce_sums_kernel(DiceBceArgs a, bool wide,
                                                                    double* __restrict__ partial) {
  const long long n = blockIdx.x / a.parts, row = n * a.M;
  const int part = blockIdx.x % a.parts;
  const bool dice = a.terms & THZ_LOSS_TERM_DICE, bce = a.terms & THZ_LOSS_TERM_BCE;
  double s_pt = 0.0, s_pp = 0.0, s_tp = 0.0, s_b = 0.0;
  for (long long c0 = (long long)part * LANE_CHUNK; c0 < a.M; c0 += (long long)a.parts * LANE_CHUNK) {
    const Lane4<true> L = sum_lane(c0, a.M, wide);
    float x[LANE_PX], t[LANE_PX], w[LANE_PX], pw[LANE_PX], b[LANE_PX];
    L.load(a.pred + row, x);
    L.load(a.target + row, t);
    fill_ones(w);
    fill_ones(pw);
    if (WEIGHTED && a.weight) L.load(a.weight + row, w);
    if (WEIGHTED && a.pos_weight) L.load(a.pos_weight + row, pw);
#pragma unroll
    for (int k = 0; k < LANE_PX; ++k) {
      b[k] = 0.0f;
      if (L.at(k) >= a.M) continue;
      if (dice) {
        s_pt += (double)x[k] * (double)t[k];
        s_pp += PK == 2 ? (double)x[k] * (double)x[k] : (double)dice_pow<PK>(x[k], a.p);
        s_tp += PK == 2 ? (double)t[k] * (double)t[k] : (double)dice_pow<PK>(t[k], a.p);
      }
      if (bce) {
        b[k] = bce_value<WEIGHTED>(x[k], t[k], w[k], pw[k]);
        s_b += (double)b[k];
      }
    }
    if (a.map) L.store(a.map + row, b);
  }
  store_partials(Sums<4>{{s_pt, s_pp, s_tp, s_b}}, partial, blockIdx.x);
}

// sums[n][k] = the parts of sample n added in index order
__global__ void __launch_bounds__(LANE_THREADS) dice_bce_finish_kernel(const double* __restrict__ partial, int parts,
                                                                      double* __restrict__ sums) {
  const Sums<4> a = gather_partials<4>(partial, parts, (long long)blockIdx.x * parts);
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) sums[(size_t)blockIdx.x * 4 + k] = a.v[k];
}

struct DiceBceGrads {
  const double* sums;   // [N][4]
  const float* g_dice;  // [N]
  const float* g_bce;   // [1], or [N M] when elementwise
  int elementwise;
  float smooth;
};

// grad_pred = g_dice[n] d/dp (1 - num / den) + g_bce d/dp bce
template <int PK, bool WEIGHTED, bool WIDE>
__global__ void __launch_bounds__(LANE_THREADS) dice_bce_bwd_kernel(DiceBceArgs a, DiceBceGrads g,
                                                                   float* __restrict__ grad) {
  const long long n = blockIdx.x / a.parts, row = n * a.M;
  const int part = blockIdx.x % a.parts;
  const bool dice = a.terms & THZ_LOSS_TERM_DICE, bce = a.terms & THZ_LOSS_TERM_BCE;
  float ct = 0.0f, cp = 0.0f, gb = 0.0f;  // the Dice term is ct t + cp d(p^e)/dp
  if (dice) {
    const double* s = g.sums + n * 4;
    const double num = s[0] + (double)g.smooth, den = s[1] + s[2] + (double)g.smooth, gd = (double)g.g_dice[n];
    ct = (float)(-gd / den);
    cp = (float)(gd * num / (den * den));
  }
  if (bce && !g.elementwise) gb = *g.g_bce;
  for (long long c0 = (long long)part * LANE_CHUNK; c0 < a.M; c0 += (long long)a.parts * LANE_CHUNK) {
    const Lane4<WIDE> L(c0, a.M);
    float x[LANE_PX], t[LANE_PX], w[LANE_PX], pw[LANE_PX], ge[LANE_PX], out[LANE_PX];
    L.load(a.pred + row, x);
    L.load(a.target + row, t);
    fill_ones(w);
    fill_ones(pw);
    if (WEIGHTED && a.weight) L.load(a.weight + row, w);
    if (WEIGHTED && a.pos_weight) L.load(a.pos_weight + row, pw);
    if (bce && g.elementwise) L.load(g.g_bce + row, ge);
#pragma unroll
    for (int k = 0; k < LANE_PX; ++k) {
      float v = 0.0f;
      if (L.at(k) < a.M) {
        if (dice) v = ct * t[k] + cp * dice_dpow<PK>(x[k], a.p);
        if (bce) v += (g.elementwise ? ge[k] : gb) * bce_slope<WEIGHTED>(x[k], t[k], w[k], pw[k]);
      }
      out[k] = v;
    }
    L.store(grad + row, out);
  }
}

#pragma clang fp contract(on)

// ---- SSIM ------------------------------------------------------------------------------------
constexpr int SS_T = 32;        // tile edge, in window positions (forward) or pixels (backward)
constexpr int SS_THREADS = 256;  // 8 rows of 32 lanes; a lane forms 4 outputs of a pass from one sliding read
constexpr int SS_R = 4;          // outputs per lane per pass

struct SsimArgs {
  int H, W, Ho, Wo;  // pixels; window positions
  int wh, ww;        // taps along H and W (1 on an axis shorter than the window)
  int nonnegative, accumulate;
  double C1, C2;
  double win[THZ_SSIM_MAX_WIN];  // the caller's taps over their fp64 sum (ssim_args)
};

__host__ __device__ inline int ss_rows(int taps) { return SS_T + taps - 1; }     // staged rows / columns
__host__ __device__ inline int ss_stride(int taps) { return ss_rows(taps) | 1; }  // odd: rows land on distinct banks
static size_t ssim_fwd_lds(int wh, int ww) {
  return (size_t)5 * ss_rows(wh) * SS_T * sizeof(double) + (size_t)2 * ss_rows(wh) * ss_stride(ww) * sizeof(float);
}
static size_t ssim_bwd_lds(int wh, int ww) {
  return (size_t)3 * ss_rows(wh) * (ss_stride(ww) + SS_T) * sizeof(float);
}

// partial[(plane tiles + tile) 2 + {0, 1}] = the tile's sums of S and of cs.  coef: [3][planes][Ho][Wo]
// (a, b, c of thz_ssim_backward) or null.
__global__ void __launch_bounds__(SS_THREADS) ssim_fwd_kernel(SsimArgs a, const float* __restrict__ x,
                                                              const float* __restrict__ y, float* __restrict__ coef,
                                                              double* __restrict__ partial) {
  extern __shared__ double ss_lds[];
  __shared__ double s_win[THZ_SSIM_MAX_WIN];
  const int tid = threadIdx.x;
  const int ih = ss_rows(a.wh), iw = ss_rows(a.ww), iwp = ss_stride(a.ww);
  double* hp = ss_lds;  // [5][ih][SS_T]
  float* xs = reinterpret_cast<float*>(hp + (size_t)5 * ih * SS_T);  // [ih][iwp]
  float* ys = xs + (size_t)ih * iwp;
  const int plane = blockIdx.z, oy = blockIdx.y * SS_T, ox = blockIdx.x * SS_T;
  const float* xp = x + (size_t)plane * a.H * a.W;
  const float* yp = y + (size_t)plane * a.H * a.W;

  if (tid < THZ_SSIM_MAX_WIN) s_win[tid] = a.win[tid];
  for (int i = tid; i < ih * iw; i += SS_THREADS) {
    const int r = i / iw, c = i - r * iw, gy = oy + r, gx = ox + c;
    const bool in = gy < a.H && gx < a.W;
    xs[r * iwp + c] = in ? xp[(size_t)gy * a.W + gx] : 0.0f;
    ys[r * iwp + c] = in ? yp[(size_t)gy * a.W + gx] : 0.0f;
  }
  __syncthreads();

  // horizontal pass: a lane forms columns c0 .. c0 + 3 of one staged row
  for (int i = tid; i < ih * (SS_T / SS_R); i += SS_THREADS) {
    const int r = i / (SS_T / SS_R), c0 = (i % (SS_T / SS_R)) * SS_R;
    double acc[SS_R][5];
#pragma unroll
    for (int o = 0; o < SS_R; ++o)
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[o][q] = 0.0;
    for (int j = 0; j < a.ww + SS_R - 1; ++j) {
      const double xv = (double)xs[r * iwp + c0 + j], yv = (double)ys[r * iwp + c0 + j];
      const double v[5] = {xv, yv, xv * xv, yv * yv, xv * yv};
#pragma unroll
      for (int o = 0; o < SS_R; ++o) {
        const int k = j - o;
        if (k < 0 || k >= a.ww) continue;
        const double w = a.ww == 1 ? 1.0 : s_win[k];
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[o][q] += w * v[q];
      }
    }
#pragma unroll
    for (int o = 0; o < SS_R; ++o)
#pragma unroll
      for (int q = 0; q < 5; ++q) hp[((size_t)q * ih + r) * SS_T + c0 + o] = acc[o][q];
  }
  __syncthreads();

  // vertical pass: a lane forms rows r0 .. r0 + 3 of one column
  const int c = tid % SS_T, r0 = (tid / SS_T) * SS_R;
  double acc[SS_R][5];
#pragma unroll
  for (int o = 0; o < SS_R; ++o)
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[o][q] = 0.0;
  for (int j = 0; j < a.wh + SS_R - 1; ++j) {
    double v[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) v[q] = hp[((size_t)q * ih + r0 + j) * SS_T + c];
#pragma unroll
    for (int o = 0; o < SS_R; ++o) {
      const int k = j - o;
      if (k < 0 || k >= a.wh) continue;
      const double w = a.wh == 1 ? 1.0 : s_win[k];
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[o][q] += w * v[q];
    }
  }

  double sum_s = 0.0, sum_cs = 0.0;
  const size_t cplane = (size_t)a.Ho * a.Wo, cstride = (size_t)gridDim.z * cplane;
#pragma unroll
  for (int o = 0; o < SS_R; ++o) {
    const int py = oy + r0 + o, px = ox + c;
    if (py >= a.Ho || px >= a.Wo) continue;
    const double mx = acc[o][0], my = acc[o][1];
    const double sx = acc[o][2] - mx * mx, sy = acc[o][3] - my * my, sxy = acc[o][4] - mx * my;
    const double A1 = 2.0 * mx * my + a.C1, A2 = 2.0 * sxy + a.C2;
    const double B1 = mx * mx + my * my + a.C1, B2 = sx + sy + a.C2;
    const double cs = A2 / B2, S = A1 / B1 * cs;
    sum_s += S;
    sum_cs += cs;
    if (coef) {
      const double ib12 = 1.0 / (B1 * B2);
      float* o3 = coef + (size_t)plane * cplane + (size_t)py * a.Wo + px;
      o3[0] = (float)(2.0 * my * (A2 - A1) * ib12 - 2.0 * mx * S * (1.0 / B1 - 1.0 / B2));
      o3[cstride] = (float)(-S / B2);
      o3[2 * cstride] = (float)(2.0 * A1 * ib12);
    }
  }
  const long long tiles = (long long)gridDim.x * gridDim.y, tile = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  store_partials(Sums<2>{{sum_s, sum_cs}}, partial, plane * tiles + tile);
}

// ssim[plane], cs[plane] = the means over the window positions; nonnegative: relu on ssim
__global__ void __launch_bounds__(LANE_THREADS) ssim_finish_kernel(const double* __restrict__ partial, int tiles,
                                                                  double positions, int nonnegative,
                                                                  float* __restrict__ ssim, float* __restrict__ cs) {
  const Sums<2> a = gather_partials<2>(partial, tiles, (long long)blockIdx.x * tiles);
  if (threadIdx.x == 0) {
    const float ms = (float)(a.v[0] / positions), mc = (float)(a.v[1] / positions);
    ssim[blockIdx.x] = nonnegative ? fmaxf(ms, 0.0f) : ms;
    if (cs) cs[blockIdx.x] = mc;
  }
}

// grad_x[p] = g[plane] / (Ho Wo) ((w * a)[p] + 2 x[p] (w * b)[p] + y[p] (w * c)[p]), * the full
// correlation over the window positions that cover pixel p.  The staged tile holds positions
// oy - (wh - 1) .. oy + 31 (zero outside the map); pixel row r gathers staged rows r + wh - 1 - u.
__global__ void __launch_bounds__(SS_THREADS) ssim_bwd_kernel(SsimArgs a, const float* __restrict__ x,
                                                              const float* __restrict__ y,
                                                              const float* __restrict__ coef,
                                                              const float* __restrict__ ssim,
                                                              const float* __restrict__ g, float* __restrict__ grad) {
  extern __shared__ double ss_lds[];
  __shared__ float s_win[THZ_SSIM_MAX_WIN];
  const int tid = threadIdx.x;
  const int ih = ss_rows(a.wh), iw = ss_rows(a.ww), iwp = ss_stride(a.ww);
  float* cs = reinterpret_cast<float*>(ss_lds);  // [3][ih][iwp]
  float* hp = cs + (size_t)3 * ih * iwp;         // [3][ih][SS_T]
  const int plane = blockIdx.z, oy = blockIdx.y * SS_T, ox = blockIdx.x * SS_T;
  const size_t cplane = (size_t)a.Ho * a.Wo, cstride = (size_t)gridDim.z * cplane;
  const float* cp = coef + (size_t)plane * cplane;

  if (tid < THZ_SSIM_MAX_WIN) s_win[tid] = (float)a.win[tid];
  for (int i = tid; i < ih * iw; i += SS_THREADS) {
    const int r = i / iw, c = i - r * iw, py = oy - (a.wh - 1) + r, px = ox - (a.ww - 1) + c;
    const bool in = py >= 0 && py < a.Ho && px >= 0 && px < a.Wo;
    const size_t at = in ? (size_t)py * a.Wo + px : 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) cs[((size_t)q * ih + r) * iwp + c] = in ? cp[q * cstride + at] : 0.0f;
  }
  __syncthreads();

  for (int i = tid; i < ih * (SS_T / SS_R); i += SS_THREADS) {
    const int r = i / (SS_T / SS_R), c0 = (i % (SS_T / SS_R)) * SS_R;
    float acc[SS_R][3];
#pragma unroll
    for (int o = 0; o < SS_R; ++o)
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[o][q] = 0.0f;
    for (int j = 0; j < a.ww + SS_R - 1; ++j) {
      float v[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) v[q] = cs[((size_t)q * ih + r) * iwp + c0 + j];
#pragma unroll
      for (int o = 0; o < SS_R; ++o) {
        const int k = a.ww - 1 - (j - o);  // staged column c0 + o + ww - 1 - k
        if (k < 0 || k >= a.ww) continue;
        const float w = a.ww == 1 ? 1.0f : s_win[k];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[o][q] += w * v[q];
      }
    }
#pragma unroll
    for (int o = 0; o < SS_R; ++o)
#pragma unroll
      for (int q = 0; q < 3; ++q) hp[((size_t)q * ih + r) * SS_T + c0 + o] = acc[o][q];
  }
  __syncthreads();

  const int c = tid % SS_T, r0 = (tid / SS_T) * SS_R;
  float acc[SS_R][3];
#pragma unroll
  for (int o = 0; o < SS_R; ++o)
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[o][q] = 0.0f;
  for (int j = 0; j < a.wh + SS_R - 1; ++j) {
    float v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = hp[((size_t)q * ih + r0 + j) * SS_T + c];
#pragma unroll
    for (int o = 0; o < SS_R; ++o) {
      const int k = a.wh - 1 - (j - o);
      if (k < 0 || k >= a.wh) continue;
      const float w = a.wh == 1 ? 1.0f : s_win[k];
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[o][q] += w * v[q];
    }
  }

  // the upstream gradient of this plane's mean; relu'(mean) = (the stored relu(mean) > 0)
  float scale = g[plane] / ((float)a.Ho * (float)a.Wo);
  if (a.nonnegative && !(ssim[plane] > 0.0f)) scale = 0.0f;
  const size_t pbase = (size_t)plane * a.H * a.W;
#pragma unroll
  for (int o = 0; o < SS_R; ++o) {
    const int gy = oy + r0 + o, gx = ox + c;
    if (gy >= a.H || gx >= a.W) continue;
    const size_t at = pbase + (size_t)gy * a.W + gx;
    const float v = scale * (acc[o][0] + 2.0f * x[at] * acc[o][1] + y[at] * acc[o][2]);
    grad[at] = a.accumulate ? grad[at] + v : v;
  }
}

// ---- host side -------------------------------------------------------------------------------
constexpr long long LOSS_MAX_N = 1LL << 24;  // samples: N parts stays far inside a grid's x extent

static int dice_bce_check(const char* who, const thz_dice_bce_desc* d) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->N < 1 || d->M < 1) return fail(THZ_E_ARG, "%s: bad shape N = %lld, M = %lld", who, d->N, d->M);
  if (d->N > LOSS_MAX_N) return fail(THZ_E_UNSUPPORTED, "%s: N = %lld > 2^24 samples", who, d->N);
  if (!(d->terms & (THZ_LOSS_TERM_DICE | THZ_LOSS_TERM_BCE)) || (d->terms & ~(THZ_LOSS_TERM_DICE | THZ_LOSS_TERM_BCE)))
    return fail(THZ_E_ARG, "%s: terms = %d", who, d->terms);
  for (const void* p : {(const void*)d->weight, (const void*)d->pos_weight})
    if (p && misaligned(p, sizeof(float))) return fail(THZ_E_ARG, "%s: weight plane misaligned", who);
  return THZ_OK;
}

// a grid that depends on (N, M) alone, so a sum's bits depend on the values only
static int dice_bce_parts(const thz_dice_bce_desc* d) {
  return partial_parts((d->M + LANE_CHUNK - 1) / LANE_CHUNK, d->N);
}
static size_t dice_bce_workspace(const thz_dice_bce_desc* d) {
  return align256(sizeof(double) * 4 * (size_t)d->N * dice_bce_parts(d));
}
static int dice_pk(float p) { return p == 1.0f ? 1 : p == 2.0f ? 2 : 0; }

template <int PK, bool WEIGHTED>
static void dice_bce_bwd_launch(bool wide, dim3 g, hipStream_t s, const DiceBceArgs& a, const DiceBceGrads& gr,
                                float* grad) {
  if (wide) hipLaunchKernelGGL((dice_bce_bwd_kernel<PK, WEIGHTED, true>), g, dim3(LANE_THREADS), 0, s, a, gr, grad);
  else hipLaunchKernelGGL((dice_bce_bwd_kernel<PK, WEIGHTED, false>), g, dim3(LANE_THREADS), 0, s, a, gr, grad);
}

// pk in {0, 1, 2} and weighted as compile-time values: f(Size<PK>{}, std::bool_constant<WEIGHTED>{})
template <class F>
static void on_dice_kind(int pk, bool weighted, F&& f) {
  auto w = [&](auto PK) {
    if (weighted) f(PK, std::true_type{});
    else f(PK, std::false_type{});
  };
  if (pk == 1) w(Size<1>{});
  else if (pk == 2) w(Size<2>{});
  else w(Size<0>{});
}

static int ssim_check(const char* who, const thz_ssim_desc* d) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->NC < 1 || d->H < 1 || d->W < 1) return fail(THZ_E_ARG, "%s: bad shape NC = %d, H = %d, W = %d", who, d->NC, d->H, d->W);
  if (d->ws < 1 || d->ws > THZ_SSIM_MAX_WIN || d->ws % 2 == 0)
    return fail(THZ_E_UNSUPPORTED, "%s: window of %d taps (odd, 1 .. %d)", who, d->ws, THZ_SSIM_MAX_WIN);
  if (d->NC > 65535 || (d->H + SS_T - 1) / SS_T > 65535)
    return fail(THZ_E_UNSUPPORTED, "%s: NC = %d planes / H = %d rows beyond the grid's extent", who, d->NC, d->H);
  return THZ_OK;
}

static SsimArgs ssim_args(const thz_ssim_desc* d) {
  SsimArgs a{};
  a.H = d->H;
  a.W = d->W;
  a.wh = d->H < d->ws ? 1 : d->ws;  // pytorch_msssim skips the filter along an axis shorter than the window
  a.ww = d->W < d->ws ? 1 : d->ws;
  a.Ho = d->H - a.wh + 1;
  a.Wo = d->W - a.ww + 1;
  a.nonnegative = d->nonnegative;
  a.accumulate = d->accumulate;
  a.C1 = d->C1;
  a.C2 = d->C2;
  // The taps reach the kernel over their own sum in fp64.  Taps normalised in fp32 sum to 1 + delta,
  // |delta| ~ 1e-8, and exact arithmetic on them turns a flat region's variance from 0 into
  // -delta x^2, which 1 / C2 amplifies a thousandfold into S; fp32 arithmetic never sees delta (the
  // sum rounds to 1), and the definition has none.
  double sum = 0.0;
  for (int k = 0; k < d->ws; ++k) sum += (double)d->window[k];
  for (int k = 0; k < THZ_SSIM_MAX_WIN; ++k) a.win[k] = k < d->ws ? (double)d->window[k] / sum : 0.0;
  return a;
}
static dim3 ssim_fwd_grid(const SsimArgs& a, int NC) {
  return dim3((unsigned)((a.Wo + SS_T - 1) / SS_T), (unsigned)((a.Ho + SS_T - 1) / SS_T), (unsigned)NC);
}
static size_t ssim_workspace(const SsimArgs& a, int NC) {
  const dim3 g = ssim_fwd_grid(a, NC);
  return align256(sizeof(double) * 2 * (size_t)g.x * g.y * g.z);
}

// The large-LDS opt-in of the two tile kernels, once (the forward crosses 64 KiB from 11 taps)
static int ssim_lds_attr() {
  static const int rc = [] {
    if (int e = lds_opt_in({(const void*)ssim_fwd_kernel}, ssim_fwd_lds(THZ_SSIM_MAX_WIN, THZ_SSIM_MAX_WIN))) return e;
    return lds_opt_in({(const void*)ssim_bwd_kernel}, ssim_bwd_lds(THZ_SSIM_MAX_WIN, THZ_SSIM_MAX_WIN));
  }();
  return rc;
}

}  // namespace thz

using namespace thz;

extern "C" int thz_dice_bce_sums_workspace_size(const thz_dice_bce_desc* d, size_t* bytes) {
  const char* who = "thz_dice_bce_sums_workspace_size";
  if (!bytes) return fail(THZ_E_ARG, "%s: null pointer", who);
  if (int e = dice_bce_check(who, d)) return e;
  *bytes = dice_bce_workspace(d);
  return THZ_OK;
}

extern "C" int thz_dice_bce_sums(const thz_dice_bce_desc* d, const float* pred, const float* target, double* sums,
                                 float* bce_map, void* workspace, size_t bytes, thz_stream_t stream) {
  const char* who = "thz_dice_bce_sums";
  if (int e = dice_bce_check(who, d)) return e;
  if (int e = check_arrays(who, {pred, target}, sizeof(float))) return e;
  if (int e = check_arrays(who, {sums, workspace}, sizeof(double))) return e;
  if (bce_map && misaligned(bce_map, sizeof(float))) return fail(THZ_E_ARG, "%s: bce_map misaligned", who);
  if (bce_map && !(d->terms & THZ_LOSS_TERM_BCE)) return fail(THZ_E_ARG, "%s: bce_map without the BCE term", who);
  if (int e = check_workspace(workspace, bytes, dice_bce_workspace(d))) return e;
  hipStream_t s = (hipStream_t)stream;
  const int parts = dice_bce_parts(d);
  const DiceBceArgs a{pred, target, d->weight, d->pos_weight, bce_map, d->M, parts, d->terms, d->p};
  const bool wide = d->M % LANE_PX == 0 && all_aligned16({pred, target, d->weight, d->pos_weight, bce_map});
  double* partial = (double*)workspace;
  const dim3 g((unsigned)(d->N * parts)), b(LANE_THREADS);
  KernelTimer kp("dice_bce_sums", s);
  on_dice_kind(dice_pk(d->p), d->weight || d->pos_weight, [&](auto PK, auto WEIGHTED) {
    hipLaunchKernelGGL((dice_bce_sums_kernel<PK(), WEIGHTED()>), g, b, 0, s, a, wide, partial);
  });
  THZ_LAUNCH_CHECK();
  kp.stop();
  KernelTimer kf("dice_bce_finish", s);
  hipLaunchKernelGGL(dice_bce_finish_kernel, dim3((unsigned)d->N), b, 0, s, (const double*)partial, parts, sums);
  THZ_LAUNCH_CHECK();
  kf.stop();
  return THZ_OK;
}

extern "C" int thz_dice_bce_backward(const thz_dice_bce_desc* d, const float* pred, const float* target,
                                     const double* sums, const float* g_dice, const float* g_bce, float* grad_pred,
                                     thz_stream_t stream) {
  const char* who = "thz_dice_bce_backward";
  if (int e = dice_bce_check(who, d)) return e;
  if (int e = check_arrays(who, {pred, target, grad_pred}, sizeof(float))) return e;
  if (d->terms & THZ_LOSS_TERM_DICE) {
    if (int e = check_arrays(who, {sums}, sizeof(double))) return e;
    if (int e = check_arrays(who, {g_dice}, sizeof(float))) return e;
  }
  if (d->terms & THZ_LOSS_TERM_BCE)
    if (int e = check_arrays(who, {g_bce}, sizeof(float))) return e;
  hipStream_t s = (hipStream_t)stream;
  const int parts = dice_bce_parts(d);
  const DiceBceArgs a{pred, target, d->weight, d->pos_weight, nullptr, d->M, parts, d->terms, d->p};
  const DiceBceGrads gr{sums, g_dice, g_bce, d->bce_grad_elementwise, d->smooth};
  const bool wide = d->M % LANE_PX == 0 &&
                    all_aligned16({pred, target, d->weight, d->pos_weight, grad_pred,
                                   d->bce_grad_elementwise && (d->terms & THZ_LOSS_TERM_BCE) ? g_bce : nullptr});
  const dim3 g((unsigned)(d->N * parts));
  KernelTimer kt("dice_bce_bwd", s);
  on_dice_kind(dice_pk(d->p), d->weight || d->pos_weight, [&](auto PK, auto WEIGHTED) {
    dice_bce_bwd_launch<PK(), WEIGHTED()>(wide, g, s, a, gr, grad_pred);
  });
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_ssim_workspace_size(const thz_ssim_desc* d, size_t* bytes) {
  const char* who = "thz_ssim_workspace_size";
  if (!bytes) return fail(THZ_E_ARG, "%s: null pointer", who);
  if (int e = ssim_check(who, d)) return e;
  *bytes = ssim_workspace(ssim_args(d), d->NC);
  return THZ_OK;
}

extern "C" int thz_ssim_forward(const thz_ssim_desc* d, const float* x, const float* y, float* ssim, float* cs,
                                float* coef, void* workspace, size_t bytes, thz_stream_t stream) {
  const char* who = "thz_ssim_forward";
  if (int e = ssim_check(who, d)) return e;
  if (int e = check_arrays(who, {x, y, ssim}, sizeof(float))) return e;
  if (int e = check_arrays(who, {workspace}, sizeof(double))) return e;
  for (const void* p : {(const void*)cs, (const void*)coef})
    if (p && misaligned(p, sizeof(float))) return fail(THZ_E_ARG, "%s: output misaligned", who);
  const SsimArgs a = ssim_args(d);
  if (int e = check_workspace(workspace, bytes, ssim_workspace(a, d->NC))) return e;
  if (int e = ssim_lds_attr()) return e;
  hipStream_t s = (hipStream_t)stream;
  const dim3 g = ssim_fwd_grid(a, d->NC);
  double* partial = (double*)workspace;
  KernelTimer kt("ssim_fwd", s);
  hipLaunchKernelGGL(ssim_fwd_kernel, g, dim3(SS_THREADS), ssim_fwd_lds(a.wh, a.ww), s, a, x, y, coef, partial);
  THZ_LAUNCH_CHECK();
  kt.stop();
  KernelTimer kf("ssim_finish", s);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)d->NC), dim3(LANE_THREADS), 0, s, (const double*)partial,
                     (int)(g.x * g.y), (double)a.Ho * (double)a.Wo, a.nonnegative, ssim, cs);
  THZ_LAUNCH_CHECK();
  kf.stop();
  return THZ_OK;
}

extern "C" int thz_ssim_backward(const thz_ssim_desc* d, const float* x, const float* y, const float* coef,
                                 const float* ssim, const float* g, float* grad_x, thz_stream_t stream) {
  const char* who = "thz_ssim_backward";
  if (int e = ssim_check(who, d)) return e;
  if (int e = check_arrays(who, {x, y, coef, ssim, g, grad_x}, sizeof(float))) return e;
  const SsimArgs a = ssim_args(d);
  if (int e = ssim_lds_attr()) return e;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((a.W + SS_T - 1) / SS_T), (unsigned)((a.H + SS_T - 1) / SS_T), (unsigned)d->NC);
  KernelTimer kt("ssim_bwd", s);
  hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(SS_THREADS), ssim_bwd_lds(a.wh, a.ww), s, a, x, y, coef, ssim, g,
                     grad_x);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
