// Zernike wavefront analysis over a circular pupil: projection, Gram matrix, synthesis and the exported table
// (include/thzdoe.h: thz_zernike_*; zernike.py, utils/metrics.py, Components/ZernikeDOE.py).  Not part of
// the reference.  Zernike polynomials are not separable in x and y, so the two-table chain of thz_modes.hip cannot
// serve them: the basis is generated per pixel, written to LDS and fed to the fp32 matrix cores from there
// (v_mfma_f32_32x32x2_f32: A 32 x 2, B 2 x 32, lane (l, h) = (lane % 32, lane / 32) holds A[l][h] and B[h][l],
// accumulator v of that lane is D[8 (v / 4) + 4 h + v % 4][l]).
//
//   strip        64 consecutive pixels of one image row.  A workgroup of four waves walks strips at a stride of the
//                grid; a strip whose row or columns miss the pupil is skipped (projection, Gram) or stored as zeros
//                (synthesis).  The projection's strips cover the pupil's bounding box only.
//   generate     zk_generate, the one device function behind all three entries: lane = pixel, wave = a group of
//                azimuthal orders |m| ({0,7,8}, {1,6,9,13}, {2,5,10,14}, {3,4,11,12}: sixteen radial polynomials each at
//                n_max = 14).  Geometry in fp64, rounded once (thzdoe.h has the contract); then the Chebyshev recurrence
//                for cos / sin(m theta), the running rho^m and the Jacobi three-term recurrence in fp32 with explicit
//                fmaf; coefficients are compile-time constants formed in double and rounded once.  The values go to
//                the LDS tile Z[128][ZK_LD]: a store instruction writes 64 consecutive floats of one row.
//   LDS stride   ZK_LD = 68 floats: rows stay 16-byte aligned, and 68 = 4 (mod 32 and mod 64), so the rows that one
//                ds_read_b128 pass touches start at every fourth bank once -- the stride-36 argument of thz_hankel.hip at
//                a 64-pixel width.  The synthesis reads single floats, 32 consecutive ones of a row per half-wave.
//   project      C[k, n] += sum_p Z[k, p] w[n, p]: wave q owns rows 32 q .. 32 q + 31 of K and all 32 planes of the
//                chunk.  A lane reads four consecutive p of its row as one b128 from the Z tile and from the map tile
//                (32 planes x 64 pixels at the same stride) and feeds four MFMAs, pixel 8 g + 4 h + s to MFMA s of group
//                g on both operands.  The map tile is loaded with 256-byte lines (a wave's load is 64 consecutive
//                floats of one plane), the next live strip's loads in flight behind the barrier.  Accumulators stay in
//                registers over all strips of the workgroup, which then writes one partial [128][32].
//   gram         the same walk with the Z tile on both operands.  Of the sixteen 32 x 32 tile pairs ten are computed:
//                wave q forms (q, (q + d) % 4) for d = 0, 1 and, for q < 2, d = 2 (3, 3, 2, 2 tiles).  The finish kernel
//                takes every element k <= k' from the tile that holds it and writes it to both places: G is exactly
//                symmetric.
//   finish       sums the workgroups' partials in ascending order in fp64 and rounds once.  The number of partials
//                follows H, W and the pupil alone, a plane is a column of the MFMA, and planes beyond 32 run as further
//                chunks on grid.y: no atomics, the same bits from every call, and a plane's bits do not depend on B.
//   synthesize   w[n, p] = sum_k a[n, k] Z[k, p]: A is the chunk's coefficients (32 planes x K, held in registers for
//                the whole walk), B the Z tile.  Wave q forms pixels 32 (q % 2) .. + 31 over the K half q / 2; the upper
//                half's accumulators go to the output tile in LDS, the lower half's are added to them, and the tile
//                [32 planes][64 pixels] is stored as 256-byte lines per plane row.  One code path for every B.
//   table        the Z tile of every strip copied to out[K][H][W]: for tests and plots.
// fp contraction is off: every fused multiply-add is written out.
#include <math.h>

#include <algorithm>

#include "thz_common.hpp"
#include "thz_launch.hpp"

#pragma clang fp contract(off)

namespace thz {

constexpr int ZK_NMAX = 14;                  // largest radial order: K = 120 <= four 32-row MFMA tiles
constexpr int ZK_KPAD = 128;
constexpr int ZK_PIX = 64;                   // pixels of a strip
constexpr int ZK_LD = ZK_PIX + 4;            // LDS row stride in floats (see above)
constexpr int ZK_PLANES = 32;                // planes of a chunk: the MFMA's other dimension
constexpr int ZK_THREADS = 256;
constexpr int ZK_PMAX = 512;                 // workgroups (partials) of a projection, two per CU
constexpr int ZK_SYN_GRID = 2048;            // workgroups of a synthesis or table launch, at most
constexpr int ZK_S = ZK_NMAX / 2 + 1;        // radial polynomials of one |m|, at most

typedef float zk_acc __attribute__((ext_vector_type(16)));

__device__ __forceinline__ zk_acc zk_zero() {
  zk_acc a;
#pragma unroll
  for (int v = 0; v < 16; ++v) a[v] = 0.0f;
  return a;
}

// ---- the recurrence's constants ---------------------------------------------------------------------
// With s = (n - m) / 2, c = 2 s + m and q_s = rho^m P_s^(0,m)(t), t = 2 rho^2 - 1:
//   q_0 = rho^m,  q_1 = ((m + 2) t - m) / 2 q_0,
//   q_s = (A t - B) q_{s-1} - C q_{s-2},  D = 2 s (s + m) (c - 2),
//   A = (c - 1) c (c - 2) / D,  B = (c - 1) m^2 / D,  C = 2 (s - 1) (s + m - 1) c / D,
// s = 1 written as A = (m + 2) / 2, B = m / 2, C = 0.  N = sqrt(n + 1) for m = 0, else sqrt(2 (n + 1)).
struct ZkTab {
  float A[ZK_NMAX + 1][ZK_S], B[ZK_NMAX + 1][ZK_S], C[ZK_NMAX + 1][ZK_S], N[ZK_NMAX + 1][ZK_S];
};

constexpr double zk_sqrt(double x) {  // Newton from above: exact to the last bit or two of a double, then rounded to fp32
  double r = x > 1.0 ? x : 1.0;
  for (int i = 0; i < 64; ++i) r = 0.5 * (r + x / r);
  return r;
}

constexpr ZkTab zk_make_tab() {
  ZkTab t{};
  for (int m = 0; m <= ZK_NMAX; ++m)
    for (int s = 0; s < ZK_S; ++s) {
      const int n = m + 2 * s;
      const double c = 2.0 * s + m, D = 2.0 * s * (s + m) * (c - 2.0);
      t.N[m][s] = (float)zk_sqrt(m == 0 ? n + 1.0 : 2.0 * (n + 1.0));
      if (s == 1) {
        t.A[m][s] = (float)((m + 2.0) / 2.0), t.B[m][s] = (float)(m / 2.0);
      } else if (s > 1) {
        t.A[m][s] = (float)((c - 1.0) * c * (c - 2.0) / D);
        t.B[m][s] = (float)((c - 1.0) * m * m / D);
        t.C[m][s] = (float)(2.0 * (s - 1.0) * (s + m - 1.0) * c / D);
      }
    }
  return t;
}

__constant__ const ZkTab zk_tab = zk_make_tab();

// the wave that generates azimuthal order m
__host__ __device__ constexpr int zk_group(int m) {
  constexpr int g[ZK_NMAX + 1] = {0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 1, 2};
  return g[m];
}

struct ZkGeom {
  double dx, dy, x0, y0, cx, cy;  // pixel (i, j) is at ((j - cx) dx - x0, (i - cy) dy - y0)
  double R2, invR;
  int H, W, nmax, K;
};

// Column `col` (= tile + pixel) of the Z tile for pixel (i, j): the rows of this wave's azimuthal orders.  Every row
// k < K of a column is written by exactly one wave; a pixel outside the pupil or the image gets zeros.
__device__ __forceinline__ void zk_generate(const ZkGeom& g, int i, int j, int wave, float* col) {
  const double x = ((double)j - g.cx) * g.dx - g.x0, y = ((double)i - g.cy) * g.dy - g.y0;
  const double r2 = x * x + y * y;
  const bool in = j < g.W && r2 <= g.R2;
  const double r = sqrt(r2), rho_d = r * g.invR;
  const double ir = r > 0.0 ? 1.0 / r : 0.0;
  const float ct = r > 0.0 ? (float)(x * ir) : 1.0f, st = (float)(y * ir);
  const float rho = (float)rho_d, t = (float)(2.0 * rho_d * rho_d - 1.0);
  const float ct2 = 2.0f * ct;
  float pm = in ? 1.0f : 0.0f;                         // rho^m, zero outside
  float cm = 1.0f, sm = 0.0f, cm1 = 0.0f, sm1 = 0.0f;  // cos / sin of m theta and of (m - 1) theta
#pragma unroll
  for (int m = 0; m <= ZK_NMAX; ++m) {
    if (m <= g.nmax) {
      if (zk_group(m) == wave) {
        float prev = 0.0f, cur = pm;
#pragma unroll
        for (int s = 0; s < ZK_S; ++s) {
          const int n = m + 2 * s;
          if (n <= ZK_NMAX && n <= g.nmax) {
            if (s > 0) {
              const float u = __builtin_fmaf(zk_tab.A[m][s], t, -zk_tab.B[m][s]);
              const float nx = __builtin_fmaf(u, cur, -(zk_tab.C[m][s] * prev));
              prev = cur, cur = nx;
            }
            const float v = zk_tab.N[m][s] * cur;
            col[((n * (n + 2) + m) / 2) * ZK_LD] = v * cm;
            if (m > 0) col[((n * (n + 2) - m) / 2) * ZK_LD] = v * sm;
          }
        }
      }
      if (m == 0) {
        cm1 = 1.0f, sm1 = 0.0f, cm = ct, sm = st;
      } else {
        const float nc = __builtin_fmaf(ct2, cm, -cm1), ns = __builtin_fmaf(ct2, sm, -sm1);
        cm1 = cm, sm1 = sm, cm = nc, sm = ns;
      }
      pm *= rho;
    }
  }
}

// whether the 64 pixels of row i from column j can hold a pupil pixel (one pixel of margin along x; exact along y:
// R^2 - y^2 < 0 exactly when y^2 > R^2)
__device__ __forceinline__ bool zk_live(const ZkGeom& g, int i, int j) {
  const double y = ((double)i - g.cy) * g.dy - g.y0;
  const double h2 = g.R2 - y * y;
  if (h2 < 0.0) return false;
  const double half = sqrt(h2) + g.dx;
  const double xa = ((double)j - g.cx) * g.dx - g.x0, xb = xa + (ZK_PIX - 1) * g.dx;
  return xa <= half && xb >= -half;
}

struct ZkArgs {
  ZkGeom g;
  const float* in;  // project: maps [B][H][W]; synthesize: coefficients [B][K]
  float* out;       // project / gram: partials; synthesize: maps [B][H][W]; table: [K][H][W]
  int B;
  int i0, j0, nseg, total;  // strip s is row i0 + s / nseg, columns j0 + 64 (s % nseg) ...
};

__device__ __forceinline__ void zk_clear(float* p, int n, int t) {
  for (int e = t; e < n; e += ZK_THREADS) p[e] = 0.0f;
}

enum { ZK_PROJECT = 0, ZK_GRAM = 1 };

template <int MODE>
__global__ void __launch_bounds__(ZK_THREADS) zk_project_kernel(ZkArgs a) {
  __shared__ __attribute__((aligned(16))) float sZ[ZK_KPAD * ZK_LD];
  __shared__ __attribute__((aligned(16))) float sW[ZK_PLANES * ZK_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int b0 = blockIdx.y * ZK_PLANES;
  const size_t HW = (size_t)a.g.H * a.g.W;
  zk_clear(sZ, ZK_KPAD * ZK_LD, t);  // rows K .. 127 stay zero
  zk_clear(sW, ZK_PLANES * ZK_LD, t);

  constexpr int NACC = MODE == ZK_GRAM ? 3 : 1;
  zk_acc acc[NACC];
#pragma unroll
  for (int d = 0; d < NACC; ++d) acc[d] = zk_zero();
  const float* pa = sZ + (wave * 32 + li) * ZK_LD + 4 * lh;
  (void)pa;  // the host pass compiles no MFMA
  (void)li;

  auto next_live = [&](int s) {
    while (s < a.total && !zk_live(a.g, a.i0 + s / a.nseg, a.j0 + ZK_PIX * (s % a.nseg))) s += gridDim.x;
    return s;
  };
  float rw[8];
  // the maps of strip s into registers: thread (pixel lane, plane wave + 4 p); absent planes and pixels are zero
  auto fetch = [&](int s) {
    const int i = a.i0 + s / a.nseg, j = a.j0 + ZK_PIX * (s % a.nseg) + lane;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int plane = b0 + wave + 4 * p;
      rw[p] = (plane < a.B && j < a.g.W) ? a.in[(size_t)plane * HW + (size_t)i * a.g.W + j] : 0.0f;
    }
  };

  int s = next_live(blockIdx.x);
  if (MODE == ZK_PROJECT && s < a.total) fetch(s);
  __syncthreads();
  while (s < a.total) {
    if (MODE == ZK_PROJECT) {
#pragma unroll
      for (int p = 0; p < 8; ++p) sW[(wave + 4 * p) * ZK_LD + lane] = rw[p];
    }
    zk_generate(a.g, a.i0 + s / a.nseg, a.j0 + ZK_PIX * (s % a.nseg) + lane, wave, sZ + lane);
    __syncthreads();
    const int sn = next_live(s + gridDim.x);
    if (MODE == ZK_PROJECT && sn < a.total) fetch(sn);
#if defined(__HIP_DEVICE_COMPILE__)
    if (wave * 32 < a.g.K) {
      if (MODE == ZK_PROJECT) {
        const float* pb = sW + li * ZK_LD + 4 * lh;
#pragma unroll
        for (int q = 0; q < ZK_PIX / 8; ++q) {
          const float4 x = *reinterpret_cast<const float4*>(pa + 8 * q);
          const float4 w = *reinterpret_cast<const float4*>(pb + 8 * q);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, w.x, acc[0], 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, w.y, acc[0], 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, w.z, acc[0], 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, w.w, acc[0], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int d = 0; d < NACC; ++d) {
          const int ct = (wave + d) & 3;
          if ((d < 2 || wave < 2) && ct * 32 < a.g.K) {
            const float* pb = sZ + (ct * 32 + li) * ZK_LD + 4 * lh;
#pragma unroll
            for (int q = 0; q < ZK_PIX / 8; ++q) {
              const float4 x = *reinterpret_cast<const float4*>(pa + 8 * q);
              const float4 w = *reinterpret_cast<const float4*>(pb + 8 * q);
              acc[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, w.x, acc[d], 0, 0, 0);
              acc[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, w.y, acc[d], 0, 0, 0);
              acc[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, w.z, acc[d], 0, 0, 0);
              acc[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, w.w, acc[d], 0, 0, 0);
            }
          }
        }
      }
    }
#endif
    __syncthreads();
    s = sn;
  }

  // one partial per workgroup: [128][32] (project, per plane chunk) or [128][128] (gram, the computed tiles)
  constexpr int PLD = MODE == ZK_GRAM ? ZK_KPAD : ZK_PLANES;
  float* P = a.out + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (ZK_KPAD * PLD);
#pragma unroll
  for (int d = 0; d < NACC; ++d) {
    if (MODE == ZK_GRAM && d == 2 && wave >= 2) continue;
    const int ct = MODE == ZK_GRAM ? ((wave + d) & 3) : 0;
#pragma unroll
    for (int v = 0; v < 16; ++v) P[(wave * 32 + 8 * (v / 4) + 4 * lh + v % 4) * PLD + ct * 32 + li] = acc[d][v];
  }
}

struct ZkFinish {
  const float* P;
  float* out;
  int B, K, parts;
};

// S[b, k]: the partials of b's chunk in ascending order, summed in fp64, rounded once
__global__ void __launch_bounds__(ZK_THREADS) zk_finish_kernel(ZkFinish f) {
  const int e = blockIdx.x * ZK_THREADS + threadIdx.x;
  if (e >= f.B * f.K) return;
  const int b = e / f.K, k = e - b * f.K;
  const float* p = f.P + (size_t)(b / ZK_PLANES) * f.parts * (ZK_KPAD * ZK_PLANES) + k * ZK_PLANES + b % ZK_PLANES;
  double s = 0.0;
  for (int q = 0; q < f.parts; ++q) s += (double)p[(size_t)q * (ZK_KPAD * ZK_PLANES)];
  f.out[e] = (float)s;
}

// G[k, k'] = G[k', k] for k <= k', from the tile that was computed: (k / 32, k' / 32), or its mirror for tile (0, 3)
__global__ void __launch_bounds__(ZK_THREADS) zk_gram_finish_kernel(ZkFinish f) {
  const int e = blockIdx.x * ZK_THREADS + threadIdx.x;
  if (e >= f.K * f.K) return;
  const int k = e / f.K, k2 = e - k * f.K;
  if (k > k2) return;
  const bool mirrored = k / 32 == 0 && k2 / 32 == 3;
  const float* p = f.P + (mirrored ? k2 * ZK_KPAD + k : k * ZK_KPAD + k2);
  double s = 0.0;
  for (int q = 0; q < f.parts; ++q) s += (double)p[(size_t)q * (ZK_KPAD * ZK_KPAD)];
  f.out[k * f.K + k2] = (float)s;
  f.out[k2 * f.K + k] = (float)s;
}

__global__ void __launch_bounds__(ZK_THREADS) zk_synthesize_kernel(ZkArgs a) {
  __shared__ __attribute__((aligned(16))) float sZ[ZK_KPAD * ZK_LD];
  __shared__ __attribute__((aligned(16))) float sO[ZK_PLANES * ZK_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int tq = wave & 1, kh = wave >> 1;  // this wave's 32 pixels of the strip and its half of K
  const int b0 = blockIdx.y * ZK_PLANES;
  const size_t HW = (size_t)a.g.H * a.g.W;
  zk_clear(sZ, ZK_KPAD * ZK_LD, t);

  // the A operand for the whole walk: MFMA s takes a[plane li][k = 64 kh + 2 s + lh]
  float ca[32];
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    const int k = 64 * kh + 2 * s + lh;
    ca[s] = (b0 + li < a.B && k < a.g.K) ? a.in[(size_t)(b0 + li) * a.g.K + k] : 0.0f;
  }
  (void)ca;  // the host pass compiles no MFMA
  const int smax = min(32, max(0, (a.g.K - 64 * kh + 1) / 2));
  (void)smax;
  (void)tq;
  __syncthreads();

  for (int s = blockIdx.x; s < a.total; s += gridDim.x) {
    const int i = a.i0 + s / a.nseg, j0 = a.j0 + ZK_PIX * (s % a.nseg);
    const bool live = zk_live(a.g, i, j0);  // the same for the whole workgroup
    if (live) {
      zk_generate(a.g, i, j0 + lane, wave, sZ + lane);
      __syncthreads();
      zk_acc o = zk_zero();
#if defined(__HIP_DEVICE_COMPILE__)
      const float* pz = sZ + (64 * kh + lh) * ZK_LD + 32 * tq + li;
#pragma unroll
      for (int q = 0; q < 32; ++q)
        if (q < smax) o = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[q], pz[2 * q * ZK_LD], o, 0, 0, 0);
#endif
      // accumulator v of lane (li, lh) is plane 8 (v / 4) + 4 lh + v % 4, pixel 32 tq + li
      float* po = sO + (4 * lh) * ZK_LD + 32 * tq + li;
      if (kh == 1) {
#pragma unroll
        for (int v = 0; v < 16; ++v) po[(8 * (v / 4) + v % 4) * ZK_LD] = o[v];
      }
      __syncthreads();
      if (kh == 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) po[(8 * (v / 4) + v % 4) * ZK_LD] = o[v] + po[(8 * (v / 4) + v % 4) * ZK_LD];
      }
      __syncthreads();
    }
    const int j = j0 + lane;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int plane = b0 + wave + 4 * p;
      if (plane < a.B && j < a.g.W)
        a.out[(size_t)plane * HW + (size_t)i * a.g.W + j] = live ? sO[(wave + 4 * p) * ZK_LD + lane] : 0.0f;
    }
  }
}

__global__ void __launch_bounds__(ZK_THREADS) zk_table_kernel(ZkArgs a) {
  __shared__ __attribute__((aligned(16))) float sZ[ZK_KPAD * ZK_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t HW = (size_t)a.g.H * a.g.W;
  for (int s = blockIdx.x; s < a.total; s += gridDim.x) {
    const int i = a.i0 + s / a.nseg, j = a.j0 + ZK_PIX * (s % a.nseg) + lane;
    zk_generate(a.g, i, j, wave, sZ + lane);
    __syncthreads();
    if (j < a.g.W)
      for (int k = wave; k < a.g.K; k += 4) a.out[(size_t)k * HW + (size_t)i * a.g.W + j] = sZ[k * ZK_LD + lane];
    __syncthreads();
  }
}

// ---- host checks and launches ---------------------------------------------------------------------
struct ZkPlan {
  ZkGeom g;
  int i0, j0, nrows, nseg;  // the pupil's bounding box in strips (nrows = 0: the pupil misses the grid)
  int parts, chunks;
};

// first and last index of an axis of n pixels that a pupil reaching [lo, hi] (in pixel units from index 0) can touch,
// one pixel of margin; false when none
static bool zk_range(double lo, double hi, int n, int* first, int* last) {
  const double a = std::max(0.0, floor(lo) - 1.0), b = std::min((double)(n - 1), ceil(hi) + 1.0);
  if (!(a <= b)) return false;
  *first = (int)a, *last = (int)b;
  return true;
}

static int zk_plan(const char* who, const thz_zernike_desc* d, ZkPlan* p) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->B < 1 || d->H < 1 || d->W < 1) return fail(THZ_E_ARG, "%s: bad shape B=%d H=%d W=%d", who, d->B, d->H, d->W);
  if (d->max_order < 0 || d->max_order > ZK_NMAX)
    return fail(THZ_E_ARG, "%s: max_order %d outside [0, %d]", who, d->max_order, ZK_NMAX);
  if (!(d->dx > 0 && d->dy > 0 && std::isfinite(d->dx) && std::isfinite(d->dy)))
    return fail(THZ_E_ARG, "%s: pitch dx=%g dy=%g must be positive", who, d->dx, d->dy);
  if (!(std::isfinite(d->x0) && std::isfinite(d->y0)))
    return fail(THZ_E_ARG, "%s: pupil centre x0=%g y0=%g must be finite", who, d->x0, d->y0);
  if (!(d->R > 0 && std::isfinite(d->R))) return fail(THZ_E_ARG, "%s: pupil radius R=%g must be positive", who, d->R);
  if ((long long)d->H * d->W > 2147483647LL)
    return fail(THZ_E_UNSUPPORTED, "%s: H W = %lld above 2^31 - 1", who, (long long)d->H * d->W);
  p->chunks = (d->B + ZK_PLANES - 1) / ZK_PLANES;
  if (p->chunks > 65535) return fail(THZ_E_UNSUPPORTED, "%s: B = %d above 32 x 65535 planes", who, d->B);
  ZkGeom& g = p->g;
  g.dx = d->dx, g.dy = d->dy, g.x0 = d->x0, g.y0 = d->y0;
  g.cx = 0.5 * (d->W - 1), g.cy = 0.5 * (d->H - 1);
  g.R2 = d->R * d->R, g.invR = 1.0 / d->R;
  g.H = d->H, g.W = d->W, g.nmax = d->max_order, g.K = (d->max_order + 1) * (d->max_order + 2) / 2;
  int i1 = 0, j1 = 0, jf = 0;
  p->nrows = p->nseg = p->i0 = p->j0 = 0;
  if (zk_range(g.cy + (d->y0 - d->R) / d->dy, g.cy + (d->y0 + d->R) / d->dy, d->H, &p->i0, &i1) &&
      zk_range(g.cx + (d->x0 - d->R) / d->dx, g.cx + (d->x0 + d->R) / d->dx, d->W, &jf, &j1)) {
    p->j0 = jf / ZK_PIX * ZK_PIX;
    p->nrows = i1 - p->i0 + 1;
    p->nseg = (j1 - p->j0) / ZK_PIX + 1;
  }
  p->parts = (int)std::max(1LL, std::min((long long)ZK_PMAX, (long long)p->nrows * p->nseg));
  return THZ_OK;
}

static size_t zk_project_bytes(const ZkPlan& p) {
  return align256((size_t)p.chunks * p.parts * ZK_KPAD * ZK_PLANES * sizeof(float));
}
static size_t zk_workspace(const ZkPlan& p, bool gram) {
  return zk_project_bytes(p) + (gram ? align256((size_t)p.parts * ZK_KPAD * ZK_KPAD * sizeof(float)) : 0);
}

// the strips of the whole image (synthesis, table)
static ZkArgs zk_image_args(const ZkPlan& p) {
  ZkArgs a{};
  a.g = p.g;
  a.nseg = (p.g.W + ZK_PIX - 1) / ZK_PIX;
  a.total = p.g.H * a.nseg;
  return a;
}

}  // namespace thz

using namespace thz;

extern "C" int thz_zernike_workspace_size(const thz_zernike_desc* d, int gram, size_t* bytes) {
  const char* who = "thz_zernike_workspace_size";
  ZkPlan p;
  if (int e = zk_plan(who, d, &p)) return e;
  if (!bytes) return fail(THZ_E_ARG, "%s: null bytes", who);
  *bytes = zk_workspace(p, gram != 0);
  return THZ_OK;
}

extern "C" int thz_zernike_project(const thz_zernike_desc* d, const float* maps, float* out, float* gram, void* workspace,
                                   size_t workspace_bytes, thz_stream_t stream) {
  const char* who = "thz_zernike_project";
  ZkPlan p;
  if (int e = zk_plan(who, d, &p)) return e;
  if (!maps != !out) return fail(THZ_E_ARG, "%s: maps and out go together", who);
  if (!maps && !gram) return fail(THZ_E_ARG, "%s: null pointer (neither maps nor gram)", who);
  if (int e = check_arrays(who, {maps ? maps : gram, out ? out : gram, gram ? gram : out}, sizeof(float))) return e;
  if (int e = check_workspace(workspace, workspace_bytes, zk_workspace(p, gram != nullptr))) return e;
  if (misaligned(workspace, 16)) return fail(THZ_E_ARG, "%s: workspace not 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  ZkArgs a{};
  a.g = p.g;
  a.B = d->B;
  a.i0 = p.i0, a.j0 = p.j0, a.nseg = std::max(1, p.nseg), a.total = p.nrows * p.nseg;
  ZkFinish f{};
  f.B = d->B, f.K = p.g.K, f.parts = p.parts;
  if (maps) {
    a.in = maps, a.out = (float*)workspace;
    {
      KernelTimer kt("zernike_project", s);
      hipLaunchKernelGGL(zk_project_kernel<ZK_PROJECT>, dim3((unsigned)p.parts, (unsigned)p.chunks), dim3(ZK_THREADS), 0, s, a);
      THZ_LAUNCH_CHECK();
      kt.stop();
    }
    f.P = a.out, f.out = out;
    KernelTimer kt("zernike_finish", s);
    hipLaunchKernelGGL(zk_finish_kernel, dim3((unsigned)((d->B * p.g.K + ZK_THREADS - 1) / ZK_THREADS)), dim3(ZK_THREADS), 0,
                       s, f);
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  if (gram) {
    a.in = nullptr, a.out = (float*)((char*)workspace + zk_project_bytes(p));
    {
      KernelTimer kt("zernike_gram", s);
      hipLaunchKernelGGL(zk_project_kernel<ZK_GRAM>, dim3((unsigned)p.parts, 1u), dim3(ZK_THREADS), 0, s, a);
      THZ_LAUNCH_CHECK();
      kt.stop();
    }
    f.P = a.out, f.out = gram;
    KernelTimer kt("zernike_gram_finish", s);
    hipLaunchKernelGGL(zk_gram_finish_kernel, dim3((unsigned)((p.g.K * p.g.K + ZK_THREADS - 1) / ZK_THREADS)),
                       dim3(ZK_THREADS), 0, s, f);
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  return THZ_OK;
}

extern "C" int thz_zernike_synthesize(const thz_zernike_desc* d, const float* coeffs, float* maps, thz_stream_t stream) {
  const char* who = "thz_zernike_synthesize";
  ZkPlan p;
  if (int e = zk_plan(who, d, &p)) return e;
  if (int e = check_arrays(who, {coeffs, maps}, sizeof(float))) return e;
  ZkArgs a = zk_image_args(p);
  a.in = coeffs, a.out = maps, a.B = d->B;
  hipStream_t s = (hipStream_t)stream;
  KernelTimer kt("zernike_synthesize", s);
  hipLaunchKernelGGL(zk_synthesize_kernel, dim3((unsigned)std::min(a.total, ZK_SYN_GRID), (unsigned)p.chunks),
                     dim3(ZK_THREADS), 0, s, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_zernike_table(const thz_zernike_desc* d, float* out, thz_stream_t stream) {
  const char* who = "thz_zernike_table";
  ZkPlan p;
  if (int e = zk_plan(who, d, &p)) return e;
  if (int e = check_arrays(who, {out}, sizeof(float))) return e;
  ZkArgs a = zk_image_args(p);
  a.out = out;
  hipStream_t s = (hipStream_t)stream;
  KernelTimer kt("zernike_table", s);
  hipLaunchKernelGGL(zk_table_kernel, dim3((unsigned)std::min(a.total, ZK_SYN_GRID)), dim3(ZK_THREADS), 0, s, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
