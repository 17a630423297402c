// The two projections of the iterative Fourier-transform algorithm (IFTA; Gerchberg-Saxton is its
// alpha = 1 form) between the fused DOE -> ASM forward and the Z-summing ASM adjoint
// (quantizationawarethzdoe_amd/ifta.py), as fused kernels that read no host value:
//
//   thz_ifta_target_stats    one pass over N planes of H x W complex64 U, the target amplitude T and the
//                            signal-window mask M: per plane S_all = sum |U|^2, S_in = sum_M |U|^2,
//                            S_TU = sum_M T |U|, S_TT = sum_M T^2 in fp64, then s = S_TU / S_TT and
//                            eff = S_in / S_all.  A workgroup owns IF_CHUNK consecutive pixels of a plane (a
//                            lane four consecutive pixels per step) and writes its four sums to the
//                            workspace (store_partials); ifta_stats_finish_kernel adds a plane's chunks
//                            in index order.  No atomics: the same input gives the same bits.
//   thz_ifta_target_project  inside M: a' = max(0, alpha s T + (1 - alpha) |U|), out = a' U / |U| (a' where
//                            |U| = 0); outside: out = beta U.  s is read from device memory.  Each pixel
//                            is formed in fp64 and rounded once; a lane reads its pixels before it writes
//                            them, so out == U is legal.
//   thz_ifta_doe_project     per DOE cell of r_h x r_w field pixels g = sum U conj(A) (the adjoint of the
//                            nearest upsampling), its phase turned into a height on the circle of
//                            circumference h_max = 2 pi / kappa and snapped to the level table where the
//                            cell lies within q x the half-gap of its nearest level.  A workgroup owns a
//                            strip of cells of one cell row: lanes run along a field row (contiguous
//                            reads), DP_RB rows of products go to LDS per barrier and the first lanes
//                            add their cell's products in row-major order.
// fp64 throughout, contraction off: the products of two float32 values are exact and every sum is the
// rounding of one add, as an fp64 restatement makes them.
#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_stream.hpp"
#include "thz_launch.hpp"

namespace thz {

#pragma clang fp contract(off)

constexpr int IF_THREADS = 256;
constexpr int IF_PX = 4;                                   // consecutive pixels per lane and step
constexpr int IF_STEPS = 4;                                // steps per workgroup
constexpr int IF_STEP = IF_THREADS * IF_PX;                // pixels per step
constexpr int IF_CHUNK = IF_STEP * IF_STEPS;               // a workgroup's pixels: 4096
constexpr int IF_SUMS = 4;                                 // S_all, S_in, S_TU, S_TT
constexpr int IF_STATS = 6;                                // ... s, eff

struct IfShape {
  long long N, HW;
  long long chunks;  // workgroups per plane
  int t_planes;      // 1: T [H, W] for every plane; else T [N, H, W]
  bool wide;         // 16-byte accesses: every pointer aligned and every plane's start with it
  double alpha, beta;
};

// the lane's four pixels from element i of a plane of HW (i < HW); zero / outside past the end
template <bool MASK>
__device__ __forceinline__ void if_load(const IfShape& s, const float2* u, const float* t, const unsigned char* m,
                                        long long i, float2 v[IF_PX], float tv[IF_PX], bool in[IF_PX]) {
  ld4(u, i, s.HW, s.wide, v);
  ld4(t, i, s.HW, s.wide, tv);
  if (MASK && s.wide && i + (IF_PX - 1) < s.HW) {  // the mask's four bytes as one access
    const unsigned rm = *reinterpret_cast<const unsigned*>(m + i);
#pragma unroll
    for (int k = 0; k < IF_PX; ++k) in[k] = ((rm >> (8 * k)) & 0xffu) != 0u;
  } else {
#pragma unroll
    for (int k = 0; k < IF_PX; ++k) in[k] = i + k < s.HW && (MASK ? m[i + k] != 0 : true);
  }
}

// partial[workgroup 4 ..] = the four sums over the workgroup's chunk of its plane
template <bool MASK>
__global__ void __launch_bounds__(IF_THREADS) ifta_stats_kernel(IfShape s, const float2* __restrict__ U,
                                                                const float* __restrict__ T,
                                                                const unsigned char* __restrict__ M,
                                                                double* __restrict__ partial) {
  const long long n = (long long)blockIdx.x / s.chunks, chunk = (long long)blockIdx.x - n * s.chunks;
  const float2* u = U + n * s.HW;
  const float* t = T + (s.t_planes > 1 ? n * s.HW : 0);
  double s_all = 0.0, s_in = 0.0, s_tu = 0.0, s_tt = 0.0;
#pragma unroll
  for (int it = 0; it < IF_STEPS; ++it) {
    const long long i = chunk * IF_CHUNK + (long long)it * IF_STEP + (long long)threadIdx.x * IF_PX;
    if (i < s.HW) {  // no barrier inside
      float2 v[IF_PX];
      float tv[IF_PX];
      bool in[IF_PX];
      if_load<MASK>(s, u, t, M, i, v, tv, in);
#pragma unroll
      for (int k = 0; k < IF_PX; ++k) {
        const double x = (double)v[k].x, y = (double)v[k].y, tk = (double)tv[k];
        const double I = x * x + y * y;
        s_all += I;
        if (in[k]) {
          s_in += I;
          s_tu += tk * sqrt(I);
          s_tt += tk * tk;
        }
      }
    }
  }
  store_partials(Sums<IF_SUMS>{{s_all, s_in, s_tu, s_tt}}, partial, blockIdx.x);
}

// out[n 6 ..]: one workgroup per plane adds the plane's chunks (gather_partials)
__global__ void __launch_bounds__(IF_THREADS) ifta_stats_finish_kernel(IfShape s, const double* __restrict__ partial,
                                                                       double* __restrict__ out) {
  const long long n = blockIdx.x;
  const Sums<IF_SUMS> sums = gather_partials<IF_SUMS>(partial, s.chunks, n * s.chunks);
  const double* a = sums.v;
  if (threadIdx.x == 0) {
    double* o = out + (size_t)n * IF_STATS;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
    o[4] = a[3] == 0.0 ? 0.0 : a[2] / a[3];
    o[5] = a[0] == 0.0 ? 0.0 : a[1] / a[0];
  }
}

// U and out may be the same array: no __restrict__ on them
template <bool MASK>
__global__ void __launch_bounds__(IF_THREADS) ifta_project_kernel(IfShape s, const float2* U, const float* __restrict__ T,
                                                                  const unsigned char* __restrict__ M,
                                                                  const double* __restrict__ scale, float2* out) {
  const long long n = (long long)blockIdx.x / s.chunks, chunk = (long long)blockIdx.x - n * s.chunks;
  const float2* u = U + n * s.HW;
  float2* o = out + n * s.HW;
  const float* t = T + (s.t_planes > 1 ? n * s.HW : 0);
  const double as = s.alpha * scale[n], om = 1.0 - s.alpha;
#pragma unroll
  for (int it = 0; it < IF_STEPS; ++it) {
    const long long i = chunk * IF_CHUNK + (long long)it * IF_STEP + (long long)threadIdx.x * IF_PX;
    if (i >= s.HW) continue;
    float2 v[IF_PX], r[IF_PX];
    float tv[IF_PX];
    bool in[IF_PX];
    if_load<MASK>(s, u, t, M, i, v, tv, in);
#pragma unroll
    for (int k = 0; k < IF_PX; ++k) {
      const double x = (double)v[k].x, y = (double)v[k].y;
      if (in[k]) {
        const double mag = sqrt(x * x + y * y);
        double a = as * (double)tv[k] + om * mag;
        a = a > 0.0 ? a : 0.0;  // NaN -> 0
        if (mag > 0.0) {
          const double f = a / mag;
          r[k] = make_float2((float)(f * x), (float)(f * y));
        } else {
          r[k] = make_float2((float)a, 0.0f);
        }
      } else {
        r[k] = make_float2((float)(s.beta * x), (float)(s.beta * y));
      }
    }
    st4(o, i, s.HW, s.wide, r);
  }
}

// ---- DOE projection --------------------------------------------------------------------------
constexpr int DP_THREADS = 256;
constexpr int DP_RB = 4;  // rows of products in LDS per barrier

struct DpArgs {
  long long N;
  int H, W, hs, ws;
  int rh, rw;     // field pixels per cell
  int cpw;        // cells per workgroup: 256 / rw, at least 1
  int strips;     // workgroups per cell row
  int nseg;       // 256-pixel segments of a cell's row: 1 unless rw > 256 (then cpw == 1)
  int a_planes;   // 0: A = 1; 1: A [H, W]; else A [N, H, W]
  int L;
  double kappa;   // the fp32 2 pi / lambda (sqrt(eps) - 1) of doe_transmission
  double hmax;    // 2 pi / kappa
  float lut[THZ_MAX_LUT];
};

// the cell's height and level from g = (gx, gy)
__device__ __forceinline__ void dp_snap(const DpArgs& a, const float* lut, double gx, double gy, double q, float* h,
                                        int* idx) {
  const double phi = (gx == 0.0 && gy == 0.0) ? 0.0 : atan2(gy, gx);
  const double v = -phi / a.kappa - (double)DOE_BASE_PLANE;
  double hc = v - floor(v / a.hmax) * a.hmax;
  if (hc >= a.hmax) hc -= a.hmax;
  if (!(hc >= 0.0)) hc = 0.0;
  // nearest level on the circle, the lowest index on a tie
  int best = 0;
  double d = __builtin_inf();
  for (int l = 0; l < a.L; ++l) {
    double dl = fabs(hc - (double)lut[l]);
    dl = fmin(dl, a.hmax - dl);
    if (dl < d) {
      d = dl;
      best = l;
    }
  }
  // the neighbour on hc's side of the level, and half the gap to it
  double off = hc - (double)lut[best];  // in (-hmax, hmax)
  if (off > 0.5 * a.hmax) off -= a.hmax;
  if (off < -0.5 * a.hmax) off += a.hmax;
  double gap;
  if (off >= 0.0) gap = best + 1 < a.L ? (double)lut[best + 1] - (double)lut[best] : (double)lut[0] + a.hmax - (double)lut[best];
  else gap = best > 0 ? (double)lut[best] - (double)lut[best - 1] : (double)lut[0] + a.hmax - (double)lut[a.L - 1];
  const bool snap = q >= 1.0 || d <= q * (0.5 * gap);
  *h = snap ? lut[best] : (float)hc;
  *idx = snap ? best : -1;
}

template <bool HAS_A>
__global__ void __launch_bounds__(DP_THREADS) ifta_doe_kernel(DpArgs a, const float2* __restrict__ U,
                                                              const float2* __restrict__ A, const float* __restrict__ q,
                                                              float* __restrict__ h, int* __restrict__ idx) {
  __shared__ double2 s_p[DP_RB][DP_THREADS];
  __shared__ float s_lut[THZ_MAX_LUT];
  const int t = threadIdx.x;
  if (t < THZ_MAX_LUT) s_lut[t] = a.lut[t < a.L ? t : a.L - 1];
  long long b = blockIdx.x;
  const int strip = (int)(b % a.strips);
  b /= a.strips;
  const int ci = (int)(b % a.hs);
  const long long n = b / a.hs;
  const int c0 = strip * a.cpw;
  const int ncell = min(a.cpw, a.ws - c0);
  const int width = a.nseg == 1 ? ncell * a.rw : a.rw;  // the strip's field columns
  const long long plane = (long long)a.H * a.W;
  const long long base = (long long)ci * a.rh * a.W + (long long)c0 * a.rw;  // inside the plane
  const float2* up = U + n * plane + base;
  const float2* ap = HAS_A ? A + (a.a_planes > 1 ? n * plane : 0) + base : nullptr;
  const int units = a.rh * a.nseg;  // a unit: one segment of one field row of the strip
  double gx = 0.0, gy = 0.0;
  for (int u0 = 0; u0 < units; u0 += DP_RB) {
#pragma unroll
    for (int k = 0; k < DP_RB; ++k) {
      const int u = u0 + k;
      double2 p = make_double2(0.0, 0.0);
      if (u < units) {
        const int r = u / a.nseg, j = (u - r * a.nseg) * DP_THREADS + t;
        if (j < width) {
          const float2 uv = up[(long long)r * a.W + j];
          const double ux = (double)uv.x, uy = (double)uv.y;
          if (HAS_A) {
            const float2 av = ap[(long long)r * a.W + j];
            const double ax = (double)av.x, ay = (double)av.y;
            p = make_double2(ux * ax + uy * ay, uy * ax - ux * ay);  // U conj(A)
          } else {
            p = make_double2(ux, uy);
          }
        }
      }
      s_p[k][t] = p;
    }
    __syncthreads();
    if (t < ncell) {
      const int lo = a.nseg == 1 ? t * a.rw : 0;
      for (int k = 0; k < DP_RB; ++k) {
        const int u = u0 + k;
        if (u >= units) break;
        const int sg = u % a.nseg;
        const int len = a.nseg == 1 ? a.rw : min(DP_THREADS, a.rw - sg * DP_THREADS);
        for (int j = 0; j < len; ++j) {
          const double2 p = s_p[k][lo + j];
          gx += p.x;
          gy += p.y;
        }
      }
    }
    __syncthreads();
  }
  if (t < ncell) {
    const long long cell = (n * a.hs + ci) * a.ws + c0 + t;
    dp_snap(a, s_lut, gx, gy, (double)q[0], h + cell, idx + cell);
  }
}

#pragma clang fp contract(on)

// ---- host side -------------------------------------------------------------------------------
constexpr long long IF_MAX_GRID = (1LL << 31) - 1;

static int if_shape(const char* who, const thz_ifta_desc* d, bool project, IfShape* s) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->N < 0 || d->H < 0 || d->W < 0)
    return fail(THZ_E_ARG, "%s: bad shape N = %lld, H = %d, W = %d", who, d->N, d->H, d->W);
  if (d->target_planes != 1 && d->target_planes != d->N)
    return fail(THZ_E_ARG, "%s: %lld target planes for N = %lld (1 or N)", who, (long long)d->target_planes, d->N);
  if (project) {
    if (!(d->alpha > 0.0 && d->alpha <= 2.0)) return fail(THZ_E_ARG, "%s: alpha %g outside (0, 2]", who, d->alpha);
    if (!(d->beta >= 0.0 && d->beta <= 1.0)) return fail(THZ_E_ARG, "%s: beta %g outside [0, 1]", who, d->beta);
  }
  s->N = d->N;
  s->HW = (long long)d->H * d->W;
  s->chunks = (s->HW + IF_CHUNK - 1) / IF_CHUNK;
  s->t_planes = d->target_planes > 1 ? 2 : 1;
  s->wide = false;
  s->alpha = d->alpha;
  s->beta = d->beta;
  if (s->chunks > 0 && d->N > IF_MAX_GRID / s->chunks)
    return fail(THZ_E_UNSUPPORTED, "%s: N = %lld planes of %d x %d beyond the grid's extent", who, d->N, d->H, d->W);
  if (d->N > IF_MAX_GRID) return fail(THZ_E_UNSUPPORTED, "%s: N = %lld planes beyond the grid's extent", who, d->N);
  return THZ_OK;
}
static size_t if_workspace(const IfShape& s) {
  return align256(sizeof(double) * IF_SUMS * (size_t)s.N * (size_t)s.chunks);
}
// 16-byte accesses need U (and out) and T 16-byte aligned, M 4-byte aligned, and every plane starting so
static bool if_planes16(const IfShape& s) { return s.HW % IF_PX == 0 || (s.N == 1 && s.t_planes == 1); }
static int if_pointers(const char* who, const void* U, const float* T, const void* out) {
  if (!U || !T || !out) return fail(THZ_E_ARG, "%s: null pointer", who);
  if (misaligned(U, 4) || misaligned(T, 4)) return fail(THZ_E_ARG, "%s: array misaligned", who);
  return THZ_OK;
}

static int dp_args(const char* who, const thz_ifta_doe_desc* d, DpArgs* a) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->N < 0 || d->H < 0 || d->W < 0 || d->hs < 0 || d->ws < 0)
    return fail(THZ_E_ARG, "%s: bad shape N = %lld, H = %d, W = %d, hs = %d, ws = %d", who, d->N, d->H, d->W, d->hs,
                d->ws);
  if (d->L < 1 || d->L > THZ_MAX_LUT) return fail(THZ_E_ARG, "%s: %d levels (1 .. %d)", who, d->L, THZ_MAX_LUT);
  if (d->incident_planes != 0 && d->incident_planes != 1 && d->incident_planes != d->N)
    return fail(THZ_E_ARG, "%s: %lld incident planes for N = %lld (0, 1 or N)", who, (long long)d->incident_planes, d->N);
  if (!(d->wavelength > 0.0f) || !(d->epsilon > 1.0f) || !std::isfinite(d->wavelength) || !std::isfinite(d->epsilon))
    return fail(THZ_E_ARG, "%s: wavelength %g, epsilon %g (wavelength > 0, epsilon > 1)", who, d->wavelength, d->epsilon);
  // kappa in fp32, in the operation order of doe_transmission
  const float k = 6.283185307179586f / d->wavelength;
  const float se = sqrtf(d->epsilon);
  const float kappa = k * (se - 1.0f);
  if (!(kappa > 0.0f) || !std::isfinite(kappa)) return fail(THZ_E_ARG, "%s: phase scale %g", who, kappa);
  a->kappa = (double)kappa;
  a->hmax = 6.283185307179586 / a->kappa;
  for (int l = 0; l < d->L; ++l) {
    const float v = d->lut[l];
    if (!(v >= 0.0f) || !((double)v < a->hmax))
      return fail(THZ_E_ARG, "%s: level %d = %g outside [0, h_max = %g)", who, l, v, a->hmax);
    if (l > 0 && !(v > d->lut[l - 1])) return fail(THZ_E_ARG, "%s: table not ascending at level %d", who, l);
  }
  // a cell is r_h x r_w whole pixels, at least one (no cells: no pixels either)
  if ((d->hs == 0 ? d->H != 0 : d->H < d->hs || d->H % d->hs != 0) ||
      (d->ws == 0 ? d->W != 0 : d->W < d->ws || d->W % d->ws != 0))
    return fail(THZ_E_UNSUPPORTED, "%s: %d x %d field over %d x %d cells: a cell must be a whole number of pixels", who,
                d->H, d->W, d->hs, d->ws);
  const bool empty = d->N == 0 || d->hs == 0 || d->ws == 0;
  a->N = d->N; a->H = d->H; a->W = d->W; a->hs = d->hs; a->ws = d->ws;
  a->rh = empty ? 1 : d->H / d->hs;
  a->rw = empty ? 1 : d->W / d->ws;
  a->cpw = a->rw >= DP_THREADS ? 1 : DP_THREADS / a->rw;
  a->nseg = a->rw > DP_THREADS ? (a->rw + DP_THREADS - 1) / DP_THREADS : 1;
  a->strips = empty ? 0 : (d->ws + a->cpw - 1) / a->cpw;
  a->a_planes = (int)(d->incident_planes > 1 ? 2 : d->incident_planes);
  a->L = d->L;
  for (int l = 0; l < THZ_MAX_LUT; ++l) a->lut[l] = l < d->L ? d->lut[l] : 0.0f;
  if (!empty && d->N > IF_MAX_GRID / ((long long)d->hs * a->strips))
    return fail(THZ_E_UNSUPPORTED, "%s: N = %lld maps of %d x %d cells beyond the grid's extent", who, d->N, d->hs, d->ws);
  return THZ_OK;
}

}  // namespace thz

using namespace thz;

extern "C" int thz_ifta_target_stats_workspace_size(const thz_ifta_desc* d, size_t* bytes) {
  const char* who = "thz_ifta_target_stats_workspace_size";
  if (!bytes) return fail(THZ_E_ARG, "%s: null pointer", who);
  IfShape sh;
  if (int e = if_shape(who, d, false, &sh)) return e;
  *bytes = if_workspace(sh);
  return THZ_OK;
}

extern "C" int thz_ifta_target_stats(const thz_ifta_desc* d, const void* U, const float* T, const unsigned char* M,
                                     double* out, void* workspace, size_t bytes, thz_stream_t stream) {
  const char* who = "thz_ifta_target_stats";
  IfShape sh;
  if (int e = if_shape(who, d, false, &sh)) return e;
  if (sh.N == 0) return THZ_OK;
  if (!out || misaligned(out, sizeof(double))) return fail(THZ_E_ARG, "%s: out null or misaligned", who);
  if (workspace && misaligned(workspace, sizeof(double))) return fail(THZ_E_ARG, "%s: workspace misaligned", who);
  hipStream_t s = (hipStream_t)stream;
  const dim3 b(IF_THREADS);
  if (sh.chunks > 0) {  // H or W == 0: the finish kernel alone writes the empty statistics
    if (int e = if_pointers(who, U, T, out)) return e;
    if (int e = check_workspace(workspace, bytes, if_workspace(sh))) return e;
    sh.wide = if_planes16(sh) && all_aligned16({U, T}) && !misaligned(M, 4);
    const dim3 g((unsigned)(sh.N * sh.chunks));
    KernelTimer kt("ifta_target_stats", s);
    if (M) hipLaunchKernelGGL(ifta_stats_kernel<true>, g, b, 0, s, sh, (const float2*)U, T, M, (double*)workspace);
    else hipLaunchKernelGGL(ifta_stats_kernel<false>, g, b, 0, s, sh, (const float2*)U, T, M, (double*)workspace);
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  KernelTimer kf("ifta_stats_finish", s);
  hipLaunchKernelGGL(ifta_stats_finish_kernel, dim3((unsigned)sh.N), b, 0, s, sh, (const double*)workspace, out);
  THZ_LAUNCH_CHECK();
  kf.stop();
  return THZ_OK;
}

extern "C" int thz_ifta_target_project(const thz_ifta_desc* d, const void* U, const float* T, const unsigned char* M,
                                       const double* scale, void* out, thz_stream_t stream) {
  const char* who = "thz_ifta_target_project";
  IfShape sh;
  if (int e = if_shape(who, d, true, &sh)) return e;
  if (sh.N == 0 || sh.chunks == 0) return THZ_OK;
  if (int e = if_pointers(who, U, T, out)) return e;
  if (!scale || misaligned(scale, sizeof(double))) return fail(THZ_E_ARG, "%s: scale null or misaligned", who);
  if (misaligned(out, 4)) return fail(THZ_E_ARG, "%s: array misaligned", who);
  sh.wide = if_planes16(sh) && all_aligned16({U, T, out}) && !misaligned(M, 4);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g((unsigned)(sh.N * sh.chunks)), b(IF_THREADS);
  KernelTimer kt("ifta_target_project", s);
  if (M) hipLaunchKernelGGL(ifta_project_kernel<true>, g, b, 0, s, sh, (const float2*)U, T, M, scale, (float2*)out);
  else hipLaunchKernelGGL(ifta_project_kernel<false>, g, b, 0, s, sh, (const float2*)U, T, M, scale, (float2*)out);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_ifta_doe_project(const thz_ifta_doe_desc* d, const void* U, const void* A, const float* q, float* h,
                                    int* idx, thz_stream_t stream) {
  const char* who = "thz_ifta_doe_project";
  DpArgs a;
  if (int e = dp_args(who, d, &a)) return e;
  if (a.strips == 0) return THZ_OK;
  if (!U || !q || !h || !idx || (a.a_planes != 0 && !A)) return fail(THZ_E_ARG, "%s: null pointer", who);
  if (misaligned(U, 4) || misaligned(A, 4) || misaligned(q, 4) || misaligned(h, 4) || misaligned(idx, 4))
    return fail(THZ_E_ARG, "%s: array misaligned", who);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g((unsigned)(a.N * a.hs * a.strips)), b(DP_THREADS);
  KernelTimer kt("ifta_doe_project", s);
  if (a.a_planes) hipLaunchKernelGGL(ifta_doe_kernel<true>, g, b, 0, s, a, (const float2*)U, (const float2*)A, q, h, idx);
  else hipLaunchKernelGGL(ifta_doe_kernel<false>, g, b, 0, s, a, (const float2*)U, (const float2*)A, q, h, idx);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
