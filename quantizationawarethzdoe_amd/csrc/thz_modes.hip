// Gaussian-mode analysis: Hermite-Gauss decomposition and synthesis (include/thzdoe.h: thz_hg_*; modes.py,
// utils/metrics.py).  Not part of the reference.  HG modes are separable, so the overlap integrals of
// a plane with M x N modes are two chained products with one real table per axis,
//
//     c[m, n] = scale sum_i sum_j Gy[m, i] U[i, j] Gx[n, j],        U[i, j] = scale sum_m sum_n Gy[m, i] c[m, n] Gx[n, j],
//
// and this unit is those products on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: A 32 x 2, B 2 x 32, lane
// (l, h) = (lane % 32, lane / 32) holds A[l][h] and B[h][l], accumulator v of that lane is D[8 (v / 4) + 4 h + v % 4][l]).
//
//   table        G [C][32][ld] float32, u_k(x_j) of thzdoe.h, built on the host in long double, rounded once and
//                cached per (device, orders, pixels, pitch, centre, waists).  Pixel coordinates are those of
//                utils/metrics.py, x_j = (j - (n_pix - 1) / 2) pitch - centre: the pixel centres of a grid whose
//                middle is the plane's centre pixel -- not the linspace(-L / 2, L / 2, n) of Guassian_beam, whose
//                pitch is L / (n - 1).  Rows at and above the order asked for are zero and ld is n_pix rounded up
//                to 128 with zeros, so no kernel guards a table access.
//   hg_analyze   A workgroup of four waves owns 128 image rows at a time, a wave 32 of them.  It streams W in LDS
//                steps of 32 columns: the U tile (de-interleaved, re and im) and the Gx tile sit at a row stride
//                of 36 floats, which keeps rows 16-byte aligned and lets the sixteen rows one ds_read_b128 pass
//                touches start at every fourth bank once (thz_hankel.hip has the argument).  A lane reads four
//                consecutive j of its row as one b128 and feeds them to four MFMAs, the j of an 8-group dealt
//                (4 h + s) to MFMA s on both operands.  The next step's global loads (8 bytes per lane, 256 bytes
//                per row) are in flight while the current one is multiplied.  T[i, n] = sum_j U[i, j] Gx[n, j] ends
//                in two accumulators (re, im) in which lane (n, h) holds rows i = 8 a + 4 h + b: exactly a B
//                operand whose k pair {8 a + b, 8 a + 4 + b} belongs to MFMA 4 a + b.  The A operand Gy[m, i] is read
//                from global memory in that order (four b128 per lane), so T never leaves the registers.  The
//                workgroup walks its row tiles with c in registers, sums its four waves through LDS in wave order
//                and writes one partial; the workgroups of a plane follow H alone, so a plane's bits do not depend
//                on B or C.
//   hg_finish    sums a plane's partials in ascending order, applies scale, interleaves re / im and crops to M x N.
//   hg_synthesize  the chain the other way.  S^T[n, i] = sum_m c[m, n] Gy[m, i] (K = 32, once per row tile) lands in
//                accumulators as the B operand of U^T[j, i] = sum_n Gx[n, j] S^T[n, i], which is streamed over W
//                with Gx read from global memory in the accumulator's order (sixteen coalesced dwords per lane,
//                the next step's in flight).  A lane then holds sixteen j of one row, so the 32 x 32 output tile is
//                transposed through LDS (row stride 33 complex) and stored as full 256-byte lines.
// No atomics: every call gives the same bits.  fp contraction is off; the products are explicit MFMA.
#include <math.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "thz_common.hpp"
#include "thz_launch.hpp"

#pragma clang fp contract(off)

namespace thz {

constexpr int MD_MAX = 32;          // orders per axis: one MFMA tile
constexpr int MD_BM = 128;          // image rows of a workgroup's tile (32 per wave)
constexpr int MD_BK = 32;           // columns of one LDS step
constexpr int MD_LD = MD_BK + 4;    // LDS row stride in floats (see above)
constexpr int MD_LDO = MD_BK + 1;   // row stride of the synthesis' output tile in complex numbers
constexpr int MD_THREADS = 256;
constexpr int MD_PMAX = 16;         // workgroups (partials) per plane: H > 2048 makes a workgroup walk several tiles
constexpr int MD_PAD = 128;         // table rows are padded to a multiple of this with zeros
constexpr long long MD_MAX_PLANES = 65535;  // grid.y

typedef float md_acc __attribute__((ext_vector_type(16)));

__device__ __forceinline__ md_acc md_zero() {
  md_acc a;
#pragma unroll
  for (int v = 0; v < 16; ++v) a[v] = 0.0f;
  return a;
}

struct MdAna {
  const float2* U;   // [planes][H][W]
  const float* Gx;   // [C][32][ldx]
  const float* Gy;   // [C][32][ldy]
  float* P;          // [planes][parts][2][32][32]
  int C, H, W, ldx, ldy, tiles;
};

__global__ void __launch_bounds__(MD_THREADS) hg_analyze_kernel(MdAna a) {
  // U re [128][36], U im [128][36], Gx [32][36]; the wave sums at the end reuse the front: [4][2][32][32]
  __shared__ __attribute__((aligned(16))) float smem[2 * MD_BM * MD_LD + MD_MAX * MD_LD];
  float* sUr = smem;
  float* sUi = smem + MD_BM * MD_LD;
  float* sG = smem + 2 * MD_BM * MD_LD;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int plane = blockIdx.y, ch = plane % a.C;
  const float2* U = a.U + (size_t)plane * a.H * a.W;
  const float* Gx = a.Gx + (size_t)ch * MD_MAX * a.ldx;
  const float* Gy = a.Gy + (size_t)ch * MD_MAX * a.ldy;
  const int u_c = t & 31, u_r = t >> 5;       // U loader: column u_c, rows u_r + 8 p
  const int g_k = (t & 7) * 4, g_n = t >> 3;  // Gx loader: order g_n, four j from g_k
  float2 ru[16];
  float4 rg;

  md_acc cre = md_zero(), cim = md_zero();
  const float* pur = sUr + (wave * 32 + li) * MD_LD + 4 * lh;
  const float* pui = sUi + (wave * 32 + li) * MD_LD + 4 * lh;
  const float* pg = sG + li * MD_LD + 4 * lh;
  (void)pur;  // the host pass compiles no MFMA
  (void)pui;
  (void)pg;

  for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int row0 = tile * MD_BM;
    // the step at j0 into registers; pixels outside the plane are zero, the table is padded
    auto fetch = [&](int j0) {
      const int j = j0 + u_c;
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        const int r = row0 + u_r + 8 * p;
        ru[p] = (r < a.H && j < a.W) ? U[(size_t)r * a.W + j] : make_float2(0.f, 0.f);
      }
      rg = *reinterpret_cast<const float4*>(Gx + (size_t)g_n * a.ldx + j0 + g_k);
    };
    // Gy[m = li][i] for the rows this lane's accumulators hold, 8 a + 4 lh + b
    float4 gy[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      gy[q] = *reinterpret_cast<const float4*>(Gy + (size_t)li * a.ldy + row0 + wave * 32 + 8 * q + 4 * lh);

    md_acc tre = md_zero(), tim = md_zero();
    (void)tre;
    (void)tim;
    (void)gy;
    fetch(0);
    for (int j0 = 0; j0 < a.W; j0 += MD_BK) {
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        sUr[(u_r + 8 * p) * MD_LD + u_c] = ru[p].x;
        sUi[(u_r + 8 * p) * MD_LD + u_c] = ru[p].y;
      }
      *reinterpret_cast<float4*>(sG + g_n * MD_LD + g_k) = rg;
      __syncthreads();
      if (j0 + MD_BK < a.W) fetch(j0 + MD_BK);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
      for (int q = 0; q < MD_BK / 8; ++q) {
        const float4 ar = *reinterpret_cast<const float4*>(pur + 8 * q);
        const float4 ai = *reinterpret_cast<const float4*>(pui + 8 * q);
        const float4 b = *reinterpret_cast<const float4*>(pg + 8 * q);
        tre = __builtin_amdgcn_mfma_f32_32x32x2f32(ar.x, b.x, tre, 0, 0, 0);
        tim = __builtin_amdgcn_mfma_f32_32x32x2f32(ai.x, b.x, tim, 0, 0, 0);
        tre = __builtin_amdgcn_mfma_f32_32x32x2f32(ar.y, b.y, tre, 0, 0, 0);
        tim = __builtin_amdgcn_mfma_f32_32x32x2f32(ai.y, b.y, tim, 0, 0, 0);
        tre = __builtin_amdgcn_mfma_f32_32x32x2f32(ar.z, b.z, tre, 0, 0, 0);
        tim = __builtin_amdgcn_mfma_f32_32x32x2f32(ai.z, b.z, tim, 0, 0, 0);
        tre = __builtin_amdgcn_mfma_f32_32x32x2f32(ar.w, b.w, tre, 0, 0, 0);
        tim = __builtin_amdgcn_mfma_f32_32x32x2f32(ai.w, b.w, tim, 0, 0, 0);
      }
#endif
      __syncthreads();
    }
    // c[m, n] += sum_i Gy[m, i] T[i, n]: accumulator v = 4 q + b of lane (n, lh) is T[8 q + 4 lh + b, n]
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cre = __builtin_amdgcn_mfma_f32_32x32x2f32(gy[q].x, tre[4 * q], cre, 0, 0, 0);
      cim = __builtin_amdgcn_mfma_f32_32x32x2f32(gy[q].x, tim[4 * q], cim, 0, 0, 0);
      cre = __builtin_amdgcn_mfma_f32_32x32x2f32(gy[q].y, tre[4 * q + 1], cre, 0, 0, 0);
      cim = __builtin_amdgcn_mfma_f32_32x32x2f32(gy[q].y, tim[4 * q + 1], cim, 0, 0, 0);
      cre = __builtin_amdgcn_mfma_f32_32x32x2f32(gy[q].z, tre[4 * q + 2], cre, 0, 0, 0);
      cim = __builtin_amdgcn_mfma_f32_32x32x2f32(gy[q].z, tim[4 * q + 2], cim, 0, 0, 0);
      cre = __builtin_amdgcn_mfma_f32_32x32x2f32(gy[q].w, tre[4 * q + 3], cre, 0, 0, 0);
      cim = __builtin_amdgcn_mfma_f32_32x32x2f32(gy[q].w, tim[4 * q + 3], cim, 0, 0, 0);
    }
#endif
  }

  // the four waves' c, summed in wave order.  The last step's barrier has released the tiles.
  float* red = smem + wave * (2 * MD_MAX * MD_MAX);
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int m = 8 * (v / 4) + 4 * lh + v % 4;
    red[m * MD_MAX + li] = cre[v];
    red[MD_MAX * MD_MAX + m * MD_MAX + li] = cim[v];
  }
  __syncthreads();
  float* P = a.P + ((size_t)plane * gridDim.x + blockIdx.x) * (2 * MD_MAX * MD_MAX);
  for (int e = t; e < 2 * MD_MAX * MD_MAX; e += MD_THREADS) {
    float s = smem[e];
#pragma unroll
    for (int w = 1; w < 4; ++w) s += smem[w * (2 * MD_MAX * MD_MAX) + e];
    P[e] = s;
  }
}

struct MdFinish {
  const float* P;
  float2* out;  // [planes][M][N]
  long long planes;
  int parts, M, N;
  float scale;
};

__global__ void __launch_bounds__(MD_THREADS) hg_finish_kernel(MdFinish f) {
  const long long total = f.planes * f.M * f.N;
  for (long long i = (long long)blockIdx.x * MD_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * MD_THREADS) {
    const int n = (int)(i % f.N), m = (int)((i / f.N) % f.M);
    const long long plane = i / ((long long)f.N * f.M);
    const float* p = f.P + (size_t)plane * f.parts * (2 * MD_MAX * MD_MAX) + m * MD_MAX + n;
    float re = 0.0f, im = 0.0f;
    for (int k = 0; k < f.parts; ++k) {
      re += p[(size_t)k * (2 * MD_MAX * MD_MAX)];
      im += p[(size_t)k * (2 * MD_MAX * MD_MAX) + MD_MAX * MD_MAX];
    }
    f.out[i] = make_float2(re * f.scale, im * f.scale);
  }
}

struct MdSyn {
  const float2* c;   // [planes][M][N]
  const float* Gx;
  const float* Gy;
  float2* U;         // [planes][H][W]
  int C, H, W, M, N, ldx, ldy;
  float scale;
};

__global__ void __launch_bounds__(MD_THREADS) hg_synthesize_kernel(MdSyn a) {
  __shared__ float2 sO[4 * MD_MAX * MD_LDO];  // a 32 x 32 output tile per wave
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int plane = blockIdx.y, ch = plane % a.C;
  const int row0 = blockIdx.x * MD_BM + wave * 32;  // below ldy: the table's rows are padded to 128
  const float2* c = a.c + (size_t)plane * a.M * a.N;
  const float* Gx = a.Gx + (size_t)ch * MD_MAX * a.ldx;
  const float* Gy = a.Gy + (size_t)ch * MD_MAX * a.ldy;
  float2* U = a.U + (size_t)plane * a.H * a.W;
  float2* so = sO + wave * (MD_MAX * MD_LDO);

  // S^T[n, i] = sum_m c[m, n] Gy[m, i]: MFMA s takes m = 2 s + lh; A is c^T (lane l = n), B is Gy (lane l = i)
  md_acc sre = md_zero(), sim = md_zero();
  (void)sre;  // the host pass compiles no MFMA
  (void)sim;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int m = 2 * s + lh;
    const float2 cv = (m < a.M && li < a.N) ? c[(size_t)m * a.N + li] : make_float2(0.f, 0.f);
    const float g = Gy[(size_t)m * a.ldy + row0 + li];
    (void)cv;
    (void)g;
#if defined(__HIP_DEVICE_COMPILE__)
    sre = __builtin_amdgcn_mfma_f32_32x32x2f32(cv.x, g, sre, 0, 0, 0);
    sim = __builtin_amdgcn_mfma_f32_32x32x2f32(cv.y, g, sim, 0, 0, 0);
#endif
  }

  // U^T[j, i] = sum_n Gx[n, j] S^T[n, i]: accumulator v = 4 q + b of lane (i, lh) is S^T[8 q + 4 lh + b, i], so MFMA v
  // takes Gx[8 q + 4 lh + b, j0 + li] as its A operand
  float gx[16], gn[16];
  auto fetch = [&](int j0, float* g) {
#pragma unroll
    for (int v = 0; v < 16; ++v) g[v] = Gx[(size_t)(8 * (v / 4) + 4 * lh + v % 4) * a.ldx + j0 + li];
  };
  fetch(0, gx);
  for (int j0 = 0; j0 < a.W; j0 += MD_BK) {
    const bool more = j0 + MD_BK < a.W;
    if (more) fetch(j0 + MD_BK, gn);
    md_acc ore = md_zero(), oim = md_zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      ore = __builtin_amdgcn_mfma_f32_32x32x2f32(gx[v], sre[v], ore, 0, 0, 0);
      oim = __builtin_amdgcn_mfma_f32_32x32x2f32(gx[v], sim[v], oim, 0, 0, 0);
    }
#endif
    // accumulator v of lane (i, lh) is U[row0 + i, j0 + 8 (v / 4) + 4 lh + v % 4]
#pragma unroll
    for (int v = 0; v < 16; ++v)
      so[li * MD_LDO + 8 * (v / 4) + 4 * lh + v % 4] = make_float2(ore[v] * a.scale, oim[v] * a.scale);
    __syncthreads();
    const int j = j0 + li;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int r = 2 * p + lh;
      if (row0 + r < a.H && j < a.W) U[(size_t)(row0 + r) * a.W + j] = so[r * MD_LDO + li];
    }
    __syncthreads();
    if (more) {
#pragma unroll
      for (int v = 0; v < 16; ++v) gx[v] = gn[v];
    }
  }
}

// ---- the table (host) ---------------------------------------------------------------------------
// u_k(x_j) of thzdoe.h for k < n_modes, j < n_pix into out[k * ld + j]; the rest of `out` is untouched
static void md_build(int n_modes, int n_pix, double pitch, double centre, double waist, float* out, size_t ld) {
  const long double r2 = sqrtl(2.0L), w = (long double)waist;
  const long double amp = sqrtl(r2 / w);
  const long double psi0 = powl(3.141592653589793238462643383279502884L, -0.25L);
  for (int j = 0; j < n_pix; ++j) {
    const long double x = ((long double)j - (long double)(n_pix - 1) / 2.0L) * (long double)pitch - (long double)centre;
    const long double xi = r2 * x / w;
    long double prev = 0.0L, cur = psi0 * expl(-xi * xi / 2.0L);
    for (int k = 0; k < n_modes; ++k) {
      out[(size_t)k * ld + j] = (float)(amp * cur);
      const long double next = sqrtl(2.0L / (k + 1)) * xi * cur - sqrtl((long double)k / (k + 1)) * prev;
      prev = cur;
      cur = next;
    }
  }
}

// ---- the per-device cache (as the Hankel table: immutable, built on first use) ----------------------
struct MdTable {
  float* G = nullptr;  // [C][32][ld]
  int ld = 0;
};
typedef std::tuple<int, int, int, double, double, std::vector<double>> MdKey;  // device, orders, pixels, pitch, centre, waists
static std::mutex g_md_mu;
static std::map<MdKey, MdTable> g_md;

static int md_ld(int n_pix) { return (n_pix + MD_PAD - 1) / MD_PAD * MD_PAD; }

static int md_table(int n_modes, int n_pix, double pitch, double centre, const double* waists, int C, MdTable* out) {
  int dev = 0;
  THZ_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_md_mu);
  const MdKey key(dev, n_modes, n_pix, pitch, centre, std::vector<double>(waists, waists + C));
  auto it = g_md.find(key);
  if (it == g_md.end()) {
    MdTable t;
    t.ld = md_ld(n_pix);
    std::vector<float> G((size_t)C * MD_MAX * t.ld, 0.0f);
    for (int c = 0; c < C; ++c) md_build(n_modes, n_pix, pitch, centre, waists[c], G.data() + (size_t)c * MD_MAX * t.ld, t.ld);
    THZ_HIP_CHECK(hipMalloc(&t.G, G.size() * sizeof(float)));
    THZ_HIP_CHECK(hipMemcpy(t.G, G.data(), G.size() * sizeof(float), hipMemcpyHostToDevice));
    it = g_md.emplace(key, t).first;
  }
  *out = it->second;
  return THZ_OK;
}

// ---- host checks and launches ---------------------------------------------------------------------
static int md_check_axis(const char* who, int n_modes, int n_pix, double pitch, double centre, const double* waists, int C) {
  if (n_modes < 1 || n_modes > MD_MAX) return fail(THZ_E_ARG, "%s: order %d outside [1, %d]", who, n_modes, MD_MAX);
  if (n_pix < 1 || C < 1) return fail(THZ_E_ARG, "%s: bad shape n_pix=%d C=%d", who, n_pix, C);
  if (!(pitch > 0.0) || !std::isfinite(pitch)) return fail(THZ_E_ARG, "%s: pitch = %g is not positive", who, pitch);
  if (!std::isfinite(centre)) return fail(THZ_E_ARG, "%s: centre = %g is not finite", who, centre);
  if (!waists) return fail(THZ_E_ARG, "%s: null waists", who);
  for (int c = 0; c < C; ++c)
    if (!(waists[c] > 0.0) || !std::isfinite(waists[c])) return fail(THZ_E_ARG, "%s: waist[%d] = %g is not positive", who, c, waists[c]);
  return THZ_OK;
}

static int md_check(const char* who, const thz_hg_desc* d) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->B < 1 || d->C < 1 || d->H < 1 || d->W < 1)
    return fail(THZ_E_ARG, "%s: bad shape B=%d C=%d H=%d W=%d", who, d->B, d->C, d->H, d->W);
  if (int e = md_check_axis(who, d->M, d->H, d->dy, d->y0, d->waist_y, d->C)) return e;
  if (int e = md_check_axis(who, d->N, d->W, d->dx, d->x0, d->waist_x, d->C)) return e;
  if (!std::isfinite(d->scale)) return fail(THZ_E_ARG, "%s: scale = %g is not finite", who, d->scale);
  if ((long long)d->B * d->C > MD_MAX_PLANES)
    return fail(THZ_E_UNSUPPORTED, "%s: B C = %lld planes > %lld", who, (long long)d->B * d->C, MD_MAX_PLANES);
  if (d->H > (1 << 30) || d->W > (1 << 30)) return fail(THZ_E_UNSUPPORTED, "%s: H=%d or W=%d above 2^30", who, d->H, d->W);
  return THZ_OK;
}

static int md_tiles(const thz_hg_desc* d) { return (d->H + MD_BM - 1) / MD_BM; }
static int md_parts(const thz_hg_desc* d) { return std::min(md_tiles(d), MD_PMAX); }
static size_t md_workspace(const thz_hg_desc* d) {
  return align256((size_t)d->B * d->C * md_parts(d) * 2 * MD_MAX * MD_MAX * sizeof(float));
}

static int md_tables(const thz_hg_desc* d, MdTable* tx, MdTable* ty) {
  if (int e = md_table(d->N, d->W, d->dx, d->x0, d->waist_x, d->C, tx)) return e;
  return md_table(d->M, d->H, d->dy, d->y0, d->waist_y, d->C, ty);
}

}  // namespace thz

using namespace thz;

extern "C" int thz_hg_workspace_size(const thz_hg_desc* d, size_t* bytes) {
  const char* who = "thz_hg_workspace_size";
  if (!bytes) return fail(THZ_E_ARG, "%s: null bytes", who);
  if (int e = md_check(who, d)) return e;
  *bytes = md_workspace(d);
  return THZ_OK;
}

extern "C" int thz_hg_analyze(const thz_hg_desc* d, const void* field, void* coeffs, void* workspace, size_t workspace_bytes,
                              thz_stream_t stream) {
  const char* who = "thz_hg_analyze";
  if (int e = md_check(who, d)) return e;
  if (int e = check_arrays(who, {field, coeffs}, sizeof(float2))) return e;
  if (int e = check_workspace(workspace, workspace_bytes, md_workspace(d))) return e;
  if (misaligned(workspace, 16)) return fail(THZ_E_ARG, "%s: workspace not 16-byte aligned", who);
  MdTable tx, ty;
  if (int e = md_tables(d, &tx, &ty)) return e;
  hipStream_t s = (hipStream_t)stream;
  const long long planes = (long long)d->B * d->C;
  MdAna a{};
  a.U = (const float2*)field; a.Gx = tx.G; a.Gy = ty.G; a.P = (float*)workspace;
  a.C = d->C; a.H = d->H; a.W = d->W; a.ldx = tx.ld; a.ldy = ty.ld; a.tiles = md_tiles(d);
  {
    KernelTimer kt("hg_analyze", s);
    hipLaunchKernelGGL(hg_analyze_kernel, dim3((unsigned)md_parts(d), (unsigned)planes), dim3(MD_THREADS), 0, s, a);
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  MdFinish f{};
  f.P = a.P; f.out = (float2*)coeffs; f.planes = planes; f.parts = md_parts(d); f.M = d->M; f.N = d->N;
  f.scale = (float)d->scale;
  int blocks = 0;
  if (int e = stream_grid((planes * d->M * d->N + MD_THREADS - 1) / MD_THREADS, &blocks)) return e;
  KernelTimer kt("hg_finish", s);
  hipLaunchKernelGGL(hg_finish_kernel, dim3((unsigned)blocks), dim3(MD_THREADS), 0, s, f);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_hg_synthesize(const thz_hg_desc* d, const void* coeffs, void* field, thz_stream_t stream) {
  const char* who = "thz_hg_synthesize";
  if (int e = md_check(who, d)) return e;
  if (int e = check_arrays(who, {coeffs, field}, sizeof(float2))) return e;
  MdTable tx, ty;
  if (int e = md_tables(d, &tx, &ty)) return e;
  hipStream_t s = (hipStream_t)stream;
  MdSyn a{};
  a.c = (const float2*)coeffs; a.Gx = tx.G; a.Gy = ty.G; a.U = (float2*)field;
  a.C = d->C; a.H = d->H; a.W = d->W; a.M = d->M; a.N = d->N; a.ldx = tx.ld; a.ldy = ty.ld;
  a.scale = (float)d->scale;
  KernelTimer kt("hg_synthesize", s);
  hipLaunchKernelGGL(hg_synthesize_kernel, dim3((unsigned)md_tiles(d), (unsigned)(d->B * d->C)), dim3(MD_THREADS), 0, s, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_hg_table_host(int n_modes, int n_pix, double pitch, double centre, const double* waists, int C, float* out) {
  const char* who = "thz_hg_table_host";
  if (int e = md_check_axis(who, n_modes, n_pix, pitch, centre, waists, C)) return e;
  if (!out) return fail(THZ_E_ARG, "%s: null pointer", who);
  for (int c = 0; c < C; ++c) md_build(n_modes, n_pix, pitch, centre, waists[c], out + (size_t)c * n_modes * n_pix, (size_t)n_pix);
  return THZ_OK;
}

extern "C" int thz_hg_table(int n_modes, int n_pix, double pitch, double centre, const double* waists, int C, float* out,
                            thz_stream_t stream) {
  const char* who = "thz_hg_table";
  if (int e = md_check_axis(who, n_modes, n_pix, pitch, centre, waists, C)) return e;
  if (int e = check_arrays(who, {out}, sizeof(float))) return e;
  MdTable t;
  if (int e = md_table(n_modes, n_pix, pitch, centre, waists, C, &t)) return e;
  hipStream_t s = (hipStream_t)stream;
  for (int c = 0; c < C; ++c)
    THZ_HIP_CHECK(hipMemcpy2DAsync(out + (size_t)c * n_modes * n_pix, (size_t)n_pix * sizeof(float),
                                   t.G + (size_t)c * MD_MAX * t.ld, (size_t)t.ld * sizeof(float), (size_t)n_pix * sizeof(float),
                                   (size_t)n_modes, hipMemcpyDeviceToDevice, s));
  return THZ_OK;
}
