// Direct Rayleigh-Sommerfeld propagation to arbitrary detector points (include/thzdoe.h: thz_rs_points_*; points.py;
// DESIGN §40).  Not part of the reference, which propagates to grids only; the kernel function is its RSC_prop's:
//
//   out[b, c, m] = dx dy sum_p U[b, c, p] G_c(x_m - x_p, y_m - y_p, z_m),
//   G_c(X, Y, z) = exp(i k_c r) z / (2 pi r^2) (1 / r - i k_c),  r = sqrt(X^2 + Y^2 + z^2),  k_c = 2 pi / lambda_c
//
// and the adjoint grad[b, c, p] = dx dy sum_m conj(G_c) g[b, c, m].  The kernel matrix is generated in registers and
// never stored; one pair-loop body, templated on the direction, serves both products.
//
//   numerical contract   geometry (X, Y, r^2, r) in fp64 from fp64 coordinates; the phase in turns, t = r (1 / lambda_c)
//                in fp64, frac(t) in fp64, rounded once to fp32, sine and cosine on that reduced argument; the
//                amplitude z / (2 pi r^2) (1 / r, -k_c) dx dy and every sum in fp32.  An fp32 phase would cost
//                1e-4 .. 1e-2 rad at k r = 1e3 .. 1e5; the fp64 part is paid once per (point, pixel) pair and shared by
//                the pair's channels and batch entries.
//   owners       live in registers: PT_OWN per lane (owner o of a workgroup's PT_WG = 512 sits on thread o % 256, slot
//                o / 256, so a slot's loads and stores are coalesced), each with its fp64 coordinates and PT_BT x PT_CT
//                complex fp32 accumulators.  Forward: owners are points.  Adjoint: owners are pixels.
//   streamed     items pass through LDS in tiles of PT_ST = 256, one per thread: fp64 (x, y, z) and the item's
//                PT_BT x PT_CT values (U of a pixel, g of a point; a value row is 256 contiguous complex numbers of
//                memory).  In the pair loop every lane reads the same LDS address: broadcasts, no bank conflict.  The
//                next tile's global loads are in flight while the current one is consumed.
//   two levels   a tile is summed into accumulators of its own that are added to the owner's totals at its end, so the
//                rounding of a sum of 10^4 .. 10^6 terms stays near that of 256; this costs 32 registers.
//   per pair     fp64: two differences, r^2, sqrt; fp32: one reciprocal and the amplitude.  Per channel: one fp64
//                multiply and fract, a conversion, sine / cosine, the complex factor.  Per batch entry: one complex FMA.
//   tiles        channels beyond PT_CT and batch entries beyond PT_BT go to grid.y; a partly filled tile skips its
//                absent channels and entries by uniform branches, and a slot that no lane of a wave fills is skipped.
//   forward split   M is often far too small to fill the device, so the pixels are cut into `chunks` contiguous
//                ranges, grid.x = point tiles x chunks; each workgroup writes its partial sums to the workspace
//                [chunks][B][C][M] and rs_points_finish adds the chunks in ascending order.  The adjoint has H W owners
//                and needs no split.  No atomics: a repeated call gives the same bits, and since a (b, c, owner) sum
//                never depends on what else shares its tile, one batch entry gives the bits it has inside a batch at
//                the same `chunks`.
//   MFMA         does not fit: the operand matrix is generated, not loaded, and each generated element is used only
//                B times -- the work is the generation, which the matrix cores cannot do.
//   sine/cosine  v_sin_f32 / v_cos_f32 take turns, which is what the reduced phase is.  THZ_POINTS_POLY selects a
//                polynomial pair on the same argument instead (A/B builds; DESIGN §40 records both).
// fp contraction is off: every fused multiply-add is written out.
#include <math.h>

#include <algorithm>

#include "thz_common.hpp"
#include "thz_launch.hpp"

#pragma clang fp contract(off)

namespace thz {

constexpr int PT_THREADS = 256;
constexpr int PT_OWN = 2;                    // owners per lane
constexpr int PT_WG = PT_THREADS * PT_OWN;   // owners of a workgroup
constexpr int PT_ST = 256;                   // items of a streamed tile
constexpr int PT_CT = 4;                     // channels of the in-lane tile
constexpr int PT_BT = 2;                     // batch entries of the in-lane tile
constexpr int PT_FILL = 1024;                // forward: workgroups wanted before the pixels stop being split
constexpr long long PT_MAX = 2147483647LL;

enum { PT_FWD = 0, PT_ADJ = 1 };

struct PtArgs {
  const float2* src;      // forward: U [B][C][HW]; adjoint: g [B][C][M]
  float2* dst;            // forward: partials [chunks][B][C][M]; adjoint: grad [B][C][HW]
  const double* points;   // [M][3]
  long long HW, M;
  long long chunk_len;    // forward: pixels of a chunk
  long long otiles;       // owner tiles (grid.x = otiles x chunks)
  int B, C, W, ctiles;
  double dx, dy, xc, yc;  // pixel (i, j) is at (xc + j dx, yc + i dy)
  float scale;            // dx dy / (2 pi)
  double inv_lam[THZ_MAX_WAVELENGTHS];
  float k[THZ_MAX_WAVELENGTHS];
};

// sine and cosine of 2 pi f for f in [0, 1]
__device__ __forceinline__ void pt_sincos_turns(float f, float* sn, float* cs) {
#if defined(THZ_POINTS_POLY)
  // quadrant q = rint(4 f), y = f - q / 4 in [-1/8, 1/8] exactly; Taylor in a = 2 pi y, |a| <= pi / 4: the sine to
  // a^9 (next term 1.7e-9), the cosine to a^8 (next term 2.4e-8), then the quadrant's swap and signs
  const float q = __builtin_rintf(4.0f * f);
  const float a = 6.2831853071795865f * __builtin_fmaf(q, -0.25f, f), a2 = a * a;
  float s = __builtin_fmaf(a2, 2.7557319e-6f, -1.9841270e-4f);
  s = __builtin_fmaf(s, a2, 8.3333333e-3f);
  s = __builtin_fmaf(s, a2, -1.6666667e-1f);
  s = __builtin_fmaf(s * a2, a, a);
  float c = __builtin_fmaf(a2, 2.4801587e-5f, -1.3888889e-3f);
  c = __builtin_fmaf(c, a2, 4.1666667e-2f);
  c = __builtin_fmaf(c, a2, -0.5f);
  c = __builtin_fmaf(c, a2, 1.0f);
  const int qi = (int)q;
  const float ss = (qi & 1) ? c : s, cc = (qi & 1) ? s : c;
  *sn = (qi & 2) ? -ss : ss;
  *cs = ((qi + 1) & 2) ? -cc : cc;
#else
  *sn = __builtin_amdgcn_sinf(f);
  *cs = __builtin_amdgcn_cosf(f);
#endif
}

// fp64 position of a pixel (z = 0) or of a point
template <bool POINT>
__device__ __forceinline__ void pt_position(const PtArgs& a, long long idx, double* x, double* y, double* z) {
  if constexpr (POINT) {
    *x = a.points[3 * idx], *y = a.points[3 * idx + 1], *z = a.points[3 * idx + 2];
  } else {
    const long long i = idx / a.W, j = idx - i * a.W;
    *x = a.xc + (double)j * a.dx, *y = a.yc + (double)i * a.dy, *z = 0.0;
  }
}

// one streamed item of a tile through registers into LDS: its position and its PT_BT x PT_CT values
template <int DIR>
struct PtStage {
  double x, y, z;
  float2 v[PT_BT * PT_CT];
  __device__ __forceinline__ void fetch(const PtArgs& a, long long item, long long end, long long n_items, int b0,
                                        int c0) {
    const bool in = item < end;
    x = y = 0.0, z = 1.0;
    if (in) pt_position<DIR == PT_ADJ>(a, item, &x, &y, &z);
#pragma unroll
    for (int b = 0; b < PT_BT; ++b)
#pragma unroll
      for (int c = 0; c < PT_CT; ++c)
        v[b * PT_CT + c] = (in && b0 + b < a.B && c0 + c < a.C)
                               ? a.src[((size_t)(b0 + b) * a.C + (c0 + c)) * n_items + item]
                               : make_float2(0.f, 0.f);
  }
  __device__ __forceinline__ void put(double* sX, double* sY, double* sZ, float2* sV, int t) const {
    sX[t] = x, sY[t] = y, sZ[t] = z;
#pragma unroll
    for (int e = 0; e < PT_BT * PT_CT; ++e) sV[t * (PT_BT * PT_CT) + e] = v[e];
  }
};

template <int DIR>
__global__ void __launch_bounds__(PT_THREADS) rs_points_kernel(PtArgs a) {
  __shared__ double sX[PT_ST], sY[PT_ST], sZ[PT_ST];
  __shared__ __attribute__((aligned(16))) float2 sV[PT_ST * PT_BT * PT_CT];
  const int t = threadIdx.x;
  const long long otile = blockIdx.x % a.otiles, chunk = blockIdx.x / a.otiles;
  const int c0 = (blockIdx.y % a.ctiles) * PT_CT, b0 = (blockIdx.y / a.ctiles) * PT_BT;
  const int nc = min(PT_CT, a.C - c0), nb = min(PT_BT, a.B - b0);
  const long long n_own = DIR == PT_FWD ? a.M : a.HW, n_items = DIR == PT_FWD ? a.HW : a.M;
  // the streamed range: the chunk's pixels, or every point
  const long long s0 = DIR == PT_FWD ? min(n_items, chunk * a.chunk_len) : 0;
  const long long s1 = DIR == PT_FWD ? min(n_items, s0 + a.chunk_len) : n_items;

  double ox[PT_OWN], oy[PT_OWN], oz[PT_OWN];
  bool live[PT_OWN];
  float2 tot[PT_OWN][PT_BT][PT_CT];
#pragma unroll
  for (int k = 0; k < PT_OWN; ++k) {
    const long long o = otile * PT_WG + k * PT_THREADS + t;
    live[k] = o < n_own;
    ox[k] = oy[k] = 0.0, oz[k] = 1.0;   // an absent owner is computed harmlessly and never stored
    if (live[k]) pt_position<DIR == PT_FWD>(a, o, &ox[k], &oy[k], &oz[k]);
#pragma unroll
    for (int b = 0; b < PT_BT; ++b)
#pragma unroll
      for (int c = 0; c < PT_CT; ++c) tot[k][b][c] = make_float2(0.f, 0.f);
  }

  PtStage<DIR> st;
  if (s0 < s1) st.fetch(a, s0 + t, s1, n_items, b0, c0);
  for (long long base = s0; base < s1; base += PT_ST) {
    st.put(sX, sY, sZ, sV, t);
    __syncthreads();
    if (base + PT_ST < s1) st.fetch(a, base + PT_ST + t, s1, n_items, b0, c0);
    const int n = (int)min((long long)PT_ST, s1 - base);
    float2 acc[PT_OWN][PT_BT][PT_CT];   // the tile's own sums: a sum of n terms is a sum of n / 256 sums of 256
#pragma unroll
    for (int k = 0; k < PT_OWN; ++k)
#pragma unroll
      for (int b = 0; b < PT_BT; ++b)
#pragma unroll
        for (int c = 0; c < PT_CT; ++c) acc[k][b][c] = make_float2(0.f, 0.f);
    for (int s = 0; s < n; ++s) {
      const double sx = sX[s], sy = sY[s], sz = sZ[s];
      float2 v[PT_BT][PT_CT];
#pragma unroll
      for (int b = 0; b < PT_BT; ++b)
#pragma unroll
        for (int c = 0; c < PT_CT; ++c)
          if (b < nb && c < nc) v[b][c] = sV[s * (PT_BT * PT_CT) + b * PT_CT + c];
#pragma unroll
      for (int k = 0; k < PT_OWN; ++k) {
        if (!__any(live[k])) continue;   // wave-uniform: a slot no lane of this wave fills
        const double X = ox[k] - sx, Y = oy[k] - sy, z = oz[k] + sz;   // one of the two z is the plane's 0
        const double r = sqrt(X * X + Y * Y + z * z);
        const float inv = __builtin_amdgcn_rcpf((float)r);
        const float amp = a.scale * (float)z * (inv * inv);
        const float ar = amp * inv;
#pragma unroll
        for (int c = 0; c < PT_CT; ++c) {
          if (c < nc) {
            const float f = (float)__builtin_amdgcn_fract(r * a.inv_lam[c0 + c]);
            const float ai = -(amp * a.k[c0 + c]);
            float sn, cs;
            pt_sincos_turns(f, &sn, &cs);
            const float fr = __builtin_fmaf(cs, ar, -(sn * ai));
            float fi = __builtin_fmaf(cs, ai, sn * ar);
            if (DIR == PT_ADJ) fi = -fi;
#pragma unroll
            for (int b = 0; b < PT_BT; ++b) {
              if (b < nb) {
                const float2 u = v[b][c];
                float2& A = acc[k][b][c];
                A.x = __builtin_fmaf(u.x, fr, __builtin_fmaf(-u.y, fi, A.x));
                A.y = __builtin_fmaf(u.x, fi, __builtin_fmaf(u.y, fr, A.y));
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < PT_OWN; ++k)
#pragma unroll
      for (int b = 0; b < PT_BT; ++b)
#pragma unroll
        for (int c = 0; c < PT_CT; ++c) tot[k][b][c].x += acc[k][b][c].x, tot[k][b][c].y += acc[k][b][c].y;
    __syncthreads();
  }

  float2* dst = a.dst + (DIR == PT_FWD ? (size_t)chunk * a.B * a.C * a.M : (size_t)0);
#pragma unroll
  for (int k = 0; k < PT_OWN; ++k) {
    const long long o = otile * PT_WG + k * PT_THREADS + t;
#pragma unroll
    for (int b = 0; b < PT_BT; ++b)
#pragma unroll
      for (int c = 0; c < PT_CT; ++c)
        if (live[k] && b < nb && c < nc) dst[((size_t)(b0 + b) * a.C + (c0 + c)) * n_own + o] = tot[k][b][c];
  }
}

// out[e] = sum of the chunks' partials of element e, in ascending chunk order
__global__ void __launch_bounds__(PT_THREADS) rs_points_finish_kernel(const float2* partial, float2* out, long long n,
                                                                      int chunks) {
  const long long e = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
  if (e >= n) return;
  float2 s = partial[e];
  for (int ch = 1; ch < chunks; ++ch) {
    const float2 p = partial[(size_t)ch * n + e];
    s.x += p.x, s.y += p.y;
  }
  out[e] = s;
}

// ---- host checks and launches ---------------------------------------------------------------------
struct PtPlan {
  long long HW, ptiles, chunk_len;
  int chunks, ctiles, btiles;
};

static int pt_plan(const char* who, const thz_points_desc* d, PtPlan* p) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->B < 1 || d->H < 1 || d->W < 1 || d->M < 1)
    return fail(THZ_E_ARG, "%s: bad shape B=%d H=%d W=%d M=%d", who, d->B, d->H, d->W, d->M);
  if (d->C < 1 || d->C > THZ_MAX_WAVELENGTHS)
    return fail(THZ_E_UNSUPPORTED, "%s: C = %d outside [1, %d]", who, d->C, THZ_MAX_WAVELENGTHS);
  if (d->chunks < 0) return fail(THZ_E_ARG, "%s: chunks = %d is negative (0: the library's choice)", who, d->chunks);
  if (!(d->dx > 0 && d->dy > 0 && std::isfinite(d->dx) && std::isfinite(d->dy)))
    return fail(THZ_E_ARG, "%s: pitch dx=%g dy=%g must be positive", who, d->dx, d->dy);
  if (!(std::isfinite(d->x0) && std::isfinite(d->y0)))
    return fail(THZ_E_ARG, "%s: origin x0=%g y0=%g must be finite", who, d->x0, d->y0);
  if (!d->wavelengths) return fail(THZ_E_ARG, "%s: null wavelengths", who);
  for (int c = 0; c < d->C; ++c)
    if (!(d->wavelengths[c] > 0 && std::isfinite(d->wavelengths[c])))
      return fail(THZ_E_ARG, "%s: wavelength[%d] = %g must be positive", who, c, (double)d->wavelengths[c]);
  p->HW = (long long)d->H * d->W;
  if (p->HW > PT_MAX) return fail(THZ_E_UNSUPPORTED, "%s: H W = %lld above 2^31 - 1", who, p->HW);
  p->ctiles = (d->C + PT_CT - 1) / PT_CT;
  p->btiles = (d->B + PT_BT - 1) / PT_BT;
  if ((long long)p->ctiles * p->btiles > 65535)
    return fail(THZ_E_UNSUPPORTED, "%s: %d x %d channel and batch tiles above 65535", who, p->ctiles, p->btiles);
  if ((long long)d->B * d->C * d->M > PT_MAX)
    return fail(THZ_E_UNSUPPORTED, "%s: B C M = %lld above 2^31 - 1", who, (long long)d->B * d->C * d->M);
  // the forward split, from the shape alone: enough chunks for PT_FILL workgroups, at most one per streamed tile
  p->ptiles = ((long long)d->M + PT_WG - 1) / PT_WG;
  const long long stiles = (p->HW + PT_ST - 1) / PT_ST;
  const long long wgs = p->ptiles * p->ctiles * p->btiles;
  long long chunks = d->chunks > 0 ? d->chunks : (PT_FILL + wgs - 1) / wgs;
  chunks = std::max(1LL, std::min(chunks, stiles));
  if (p->ptiles * chunks > PT_MAX)
    return fail(THZ_E_UNSUPPORTED, "%s: %lld point tiles x %lld chunks above 2^31 - 1", who, p->ptiles, chunks);
  p->chunks = (int)chunks;
  p->chunk_len = (p->HW + chunks - 1) / chunks;
  return THZ_OK;
}

static size_t pt_workspace(const thz_points_desc* d, const PtPlan& p) {
  return align256((size_t)p.chunks * d->B * d->C * d->M * sizeof(float2));
}

static PtArgs pt_args(const thz_points_desc* d, const PtPlan& p, const double* points) {
  PtArgs a{};
  a.points = points;
  a.HW = p.HW, a.M = d->M;
  a.B = d->B, a.C = d->C, a.W = d->W, a.ctiles = p.ctiles;
  a.dx = d->dx, a.dy = d->dy;
  a.xc = d->x0 - 0.5 * (d->W - 1) * d->dx;
  a.yc = d->y0 - 0.5 * (d->H - 1) * d->dy;
  a.scale = (float)(d->dx * d->dy / 6.283185307179586);
  for (int c = 0; c < d->C; ++c) {
    a.inv_lam[c] = 1.0 / (double)d->wavelengths[c];
    a.k[c] = (float)(6.283185307179586 / (double)d->wavelengths[c]);
  }
  return a;
}

}  // namespace thz

using namespace thz;

extern "C" int thz_rs_points_workspace_size(const thz_points_desc* d, size_t* bytes) {
  PtPlan p;
  if (int e = pt_plan("thz_rs_points_workspace_size", d, &p)) return e;
  if (!bytes) return fail(THZ_E_ARG, "thz_rs_points_workspace_size: null pointer");
  *bytes = pt_workspace(d, p);
  return THZ_OK;
}

extern "C" int thz_rs_points_forward(const thz_points_desc* d, const void* field, const double* points, void* out,
                                     void* workspace, size_t workspace_bytes, thz_stream_t stream) {
  const char* who = "thz_rs_points_forward";
  PtPlan p;
  if (int e = pt_plan(who, d, &p)) return e;
  if (int e = check_arrays(who, {field, points, out, workspace}, 8)) return e;
  if (int e = check_workspace(workspace, workspace_bytes, pt_workspace(d, p))) return e;
  PtArgs a = pt_args(d, p, points);
  a.src = (const float2*)field;
  a.dst = (float2*)workspace;
  a.chunk_len = p.chunk_len;
  a.otiles = p.ptiles;
  hipStream_t s = (hipStream_t)stream;
  {
    KernelTimer kt("rs_points_fwd", s);
    hipLaunchKernelGGL(rs_points_kernel<PT_FWD>, dim3((unsigned)(p.ptiles * p.chunks), (unsigned)(p.ctiles * p.btiles)),
                       dim3(PT_THREADS), 0, s, a);
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  const long long n = (long long)d->B * d->C * d->M;
  KernelTimer kt("rs_points_finish", s);
  hipLaunchKernelGGL(rs_points_finish_kernel, dim3((unsigned)((n + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0,
                     s, (const float2*)workspace, (float2*)out, n, p.chunks);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_rs_points_adjoint(const thz_points_desc* d, const void* grad_out, const double* points,
                                     void* grad_field, thz_stream_t stream) {
  const char* who = "thz_rs_points_adjoint";
  PtPlan p;
  if (int e = pt_plan(who, d, &p)) return e;
  if (int e = check_arrays(who, {grad_out, points, grad_field}, 8)) return e;
  PtArgs a = pt_args(d, p, points);
  a.src = (const float2*)grad_out;
  a.dst = (float2*)grad_field;
  a.otiles = (p.HW + PT_WG - 1) / PT_WG;
  hipStream_t s = (hipStream_t)stream;
  KernelTimer kt("rs_points_adj", s);
  hipLaunchKernelGGL(rs_points_kernel<PT_ADJ>, dim3((unsigned)a.otiles, (unsigned)(p.ctiles * p.btiles)),
                     dim3(PT_THREADS), 0, s, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
