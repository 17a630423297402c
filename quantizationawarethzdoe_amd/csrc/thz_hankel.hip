// Hankel propagator for rotationally symmetric fields (include/thzdoe.h: thz_hankel_*; hankel.py,
// Props/Hankel_Prop.py).  Not part of the reference: the quasi-discrete Hankel transform of
// Guizar-Sicairos & Gutierrez-Vega (2004) turns a z-sweep of a radial profile into two dense products with one
// real symmetric table T, and this unit is those products on the fp32 matrix cores.
//
//   table        T, w and the zeros of J0 are built on the host in long double (glibc j0l / j1l; zeros by
//                McMahon's expansion and four Newton steps), rounded once, and cached per (N, device).  The
//                device copy of T has its rows padded to a multiple of four floats so that every tile load
//                is one aligned 16-byte access.
//   hankel_tf    H [Z, C, N] complex64, the phase z sqrt(k^2 - kappa^2) formed and reduced in fp64.
//   hankel_gemm  Y[r, col] = sum_k T[r, k] pre[k] X[k, col] (H[z(col), c(col), k] or 1), one kernel for the
//                four products of the forward and the adjoint.  A workgroup of four waves owns 128 rows x
//                32 NT real columns (NT = 1, 2, 4: a complex column is two real ones) of one K range; a wave
//                owns 32 rows and NT accumulators of v_mfma_f32_32x32x2_f32 (16 NT VGPRs).  T tiles (128 x
//                32) and right-hand-side tiles (32 x 32 NT, transposed) go through LDS at a row stride of 36
//                floats: rows stay 16-byte aligned, and the sixteen rows one ds_read_b128 pass touches start
//                at banks 36 i mod 64 = every multiple of four once, so the reads are conflict-free.  A lane
//                reads four consecutive k of its row as one b128 and feeds them to four MFMAs; the k of an
//                8-group are dealt (4 h + s) to MFMA s, half-wave h on both operands, which permutes the
//                order of a sum and nothing else.  The next tile's global loads are in flight while the
//                current one is multiplied (register prefetch, one LDS image, two barriers per step).  The
//                loader applies pre, H and the complex product, so H (.) F is never in memory.
//   hankel_finish  sums the K splits of the workspace in ascending order, applies post[r] and interleaves
//                re / im; the adjoint's form multiplies by conj(H) and sums the Z planes in ascending order.
// No atomics: every call gives the same bits.  fp contraction is off in this unit so that the fp64 phase is
// the formula of thzdoe.h operation by operation; the products use explicit fmaf and MFMA.
#include <math.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "thz_common.hpp"
#include "thz_launch.hpp"

#pragma clang fp contract(off)

namespace thz {

constexpr int HK_MAX_N = 8192;
constexpr int HK_BM = 128;       // rows of a workgroup's tile (32 per wave)
constexpr int HK_BK = 32;        // k of one LDS step
constexpr int HK_LD = HK_BK + 4; // LDS row stride in floats (see above)
constexpr int HK_THREADS = 256;
constexpr int HK_KMIN = 128;     // a K split is no shorter than this: N = 129 is the first size that splits
constexpr int HK_TARGET = 512;   // workgroups the split aims for: two per compute unit of a 256-CU device

enum { HK_ONE = 0, HK_W = 1, HK_WINV = 2 };  // pre[k] / post[r]: 1, w, 1 / w

typedef float hk_acc __attribute__((ext_vector_type(16)));

struct HkGemm {
  const float* T;    // [N][ldT], rows padded with zeros
  const float* w;    // [N]
  const float2* X;   // [columns][K] complex
  const float2* H;   // [Z][C][N] (HMODE)
  float* P;          // [S][2 ncc][Mp] partial sums
  int ldT, M, K, ncc, Mp, kc, pre;
  int BC, C;         // HMODE: column cc = z BC + bc reads X[bc] and H[z, bc % C]
};

__device__ __forceinline__ float hk_scale(int mode, const float* w, int i) {
  return mode == HK_W ? w[i] : mode == HK_WINV ? 1.0f / w[i] : 1.0f;
}

template <int NT, bool HMODE>
__global__ void __launch_bounds__(HK_THREADS) hankel_gemm_kernel(HkGemm a) {
  __shared__ __attribute__((aligned(16))) float sA[HK_BM * HK_LD];
  __shared__ __attribute__((aligned(16))) float sB[32 * NT * HK_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row0 = blockIdx.x * HK_BM;
  const int cc0 = blockIdx.y * (16 * NT);
  const int ks = blockIdx.z * a.kc, ke = min(a.K, ks + a.kc);
  const int a_k = (t & 7) * 4, a_r = t >> 3;  // T loader: rows a_r + 32 j, four k from a_k
  const int b_k = t & 31, b_c = t >> 5;       // X loader: k = b_k, complex columns b_c + 8 j
  float4 ra[4];
  float2 rb[2 * NT];

  // the tile at k0 into registers; everything outside (M, [ks, ke), ncc) is zero.  A float4 of T that
  // straddles ke reads valid (padded) memory and meets zeros of X.
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = row0 + a_r + 32 * j, k = k0 + a_k;
      ra[j] = (r < a.M && k < ke) ? *reinterpret_cast<const float4*>(a.T + (size_t)r * a.ldT + k)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int k = k0 + b_k;
#pragma unroll
    for (int j = 0; j < 2 * NT; ++j) {
      const int cc = cc0 + b_c + 8 * j;
      float2 v = make_float2(0.f, 0.f);
      if (k < ke && cc < a.ncc) {
        if (HMODE) {
          const int z = cc / a.BC, bc = cc - z * a.BC;
          const float2 x = a.X[(size_t)bc * a.K + k];
          const float2 h = a.H[((size_t)z * a.C + bc % a.C) * a.K + k];
          v = make_float2(fmaf(h.x, x.x, -(h.y * x.y)), fmaf(h.x, x.y, h.y * x.x));
        } else {
          v = a.X[(size_t)cc * a.K + k];
        }
        const float s = hk_scale(a.pre, a.w, k);
        v = make_float2(v.x * s, v.y * s);
      }
      rb[j] = v;
    }
  };

  hk_acc acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[n][v] = 0.0f;

  const int li = lane & 31, lh = lane >> 5;
  const float* pa = sA + (wave * 32 + li) * HK_LD + 4 * lh;
  const float* pb = sB + li * HK_LD + 4 * lh;
  (void)pa;  // the host pass compiles no MFMA
  (void)pb;
  fetch(ks);
  for (int k0 = ks; k0 < ke; k0 += HK_BK) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(sA + (a_r + 32 * j) * HK_LD + a_k) = ra[j];
#pragma unroll
    for (int j = 0; j < 2 * NT; ++j) {
      const int c = b_c + 8 * j;
      sB[(2 * c) * HK_LD + b_k] = rb[j].x;
      sB[(2 * c + 1) * HK_LD + b_k] = rb[j].y;
    }
    __syncthreads();
    if (k0 + HK_BK < ke) fetch(k0 + HK_BK);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int q = 0; q < HK_BK / 8; ++q) {
      const float4 av = *reinterpret_cast<const float4*>(pa + 8 * q);
      float4 bv[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) bv[n] = *reinterpret_cast<const float4*>(pb + n * 32 * HK_LD + 8 * q);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[n].x, acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[n].y, acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[n].z, acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[n].w, acc[n], 0, 0, 0);
    }
#endif
    __syncthreads();
  }

  // accumulator v of lane (li, lh) is row 8 (v / 4) + 4 lh + v % 4, column li of its 32 x 32 tile
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = 2 * cc0 + 32 * n + li;
    if (col >= 2 * a.ncc) continue;
    float* p = a.P + ((size_t)blockIdx.z * (2 * a.ncc) + col) * a.Mp;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int r = row0 + wave * 32 + 8 * g + 4 * lh;
      if (r + 3 < a.M) {
        *reinterpret_cast<float4*>(p + r) = make_float4(acc[n][4 * g], acc[n][4 * g + 1], acc[n][4 * g + 2], acc[n][4 * g + 3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (r + e < a.M) p[r + e] = acc[n][4 * g + e];
      }
    }
  }
}

struct HkFinish {
  const float* P;
  const float* w;
  const float2* H;  // ZSUM: [Z][C][M]
  float2* out;      // [ncc][M], or [BC][M] (ZSUM)
  int S, ncc, Mp, M, post, Z, BC, C;
};

// the K splits of one real column at row r, summed in ascending order
__device__ __forceinline__ float hk_splits(const HkFinish& f, int col, int r) {
  float s = 0.0f;
  for (int i = 0; i < f.S; ++i) s += f.P[((size_t)i * (2 * f.ncc) + col) * f.Mp + r];
  return s;
}

template <bool ZSUM>
__global__ void __launch_bounds__(HK_THREADS) hankel_finish_kernel(HkFinish f) {
  const long long total = (long long)(ZSUM ? f.BC : f.ncc) * f.M;
  for (long long i = (long long)blockIdx.x * HK_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * HK_THREADS) {
    const int co = (int)(i / f.M), r = (int)(i - (long long)co * f.M);
    if (ZSUM) {  // sum_z conj(H[z, c, r]) g'[z, bc, r]
      float ax = 0.0f, ay = 0.0f;
      for (int z = 0; z < f.Z; ++z) {
        const int cc = z * f.BC + co;
        const float re = hk_splits(f, 2 * cc, r), im = hk_splits(f, 2 * cc + 1, r);
        const float2 h = f.H[((size_t)z * f.C + co % f.C) * f.M + r];
        ax = fmaf(h.x, re, fmaf(h.y, im, ax));
        ay = fmaf(h.x, im, fmaf(-h.y, re, ay));
      }
      f.out[i] = make_float2(ax, ay);
    } else {
      const float s = hk_scale(f.post, f.w, r);
      f.out[i] = make_float2(hk_splits(f, 2 * co, r) * s, hk_splits(f, 2 * co + 1, r) * s);
    }
  }
}

struct HkTf {
  int Z, C, N;
  double r_max;
  const double* zeros;
  const float* z_dev;
  float2* H;
  float z[THZ_MAX_Z];
  float lam[THZ_MAX_WAVELENGTHS];
};

// H[z, c, m] of thzdoe.h; every fp64 operation rounded once, in the order written there
__global__ void __launch_bounds__(HK_THREADS) hankel_tf_kernel(HkTf a) {
  const long long total = (long long)a.Z * a.C * a.N;
  for (long long i = (long long)blockIdx.x * HK_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * HK_THREADS) {
    const int m = (int)(i % a.N), c = (int)((i / a.N) % a.C), z = (int)(i / ((long long)a.N * a.C));
    const double k = 6.283185307179586 / (double)a.lam[c];
    const double kap = a.zeros[m] / a.r_max;
    float2 h = make_float2(0.f, 0.f);
    if (kap < k) {
      const double zz = (double)(a.z_dev ? a.z_dev[z] : a.z[z]);
      const double ph = zz * sqrt(k * k - kap * kap);
      double sn, cs;
      sincos(ph, &sn, &cs);
      h = make_float2((float)cs, (float)sn);
    }
    a.H[i] = h;
  }
}

// ---- the table (host) ---------------------------------------------------------------------------
// zeros [N + 1], w [N] and T [N][ld] of thzdoe.h.  T is symmetric: a thread forms the upper part of its rows
// and mirrors it.
static void hk_build(int N, int ld, std::vector<double>* zeros, std::vector<float>* w, std::vector<float>* T) {
  zeros->assign(N + 1, 0.0);
  for (int s = 1; s <= N + 1; ++s) {
    const long double b = (s - 0.25L) * 3.141592653589793238462643383279502884L, b8 = 8 * b;
    long double x = b + 1 / b8 - 124 / (3 * b8 * b8 * b8) + 120928 / (15 * b8 * b8 * b8 * b8 * b8);  // McMahon
    for (int it = 0; it < 4; ++it) x += ::j0l(x) / ::j1l(x);  // Newton: J0' = -J1
    (*zeros)[s - 1] = (double)x;
  }
  std::vector<long double> aj1(N);
  w->assign(N, 0.0f);
  for (int m = 0; m < N; ++m) {
    aj1[m] = fabsl(::j1l((long double)(*zeros)[m]));
    (*w)[m] = (float)(1.0L / aj1[m]);
  }
  T->assign((size_t)N * ld, 0.0f);
  const double S = (*zeros)[N];
  const double* j = zeros->data();
  float* Tp = T->data();
  const int nth = (int)std::max(1u, std::min(16u, std::min(std::thread::hardware_concurrency(), (unsigned)(N / 64 + 1))));
  auto rows = [&](int first) {
    for (int m = first; m < N; m += nth)
      for (int n = m; n < N; ++n) {
        const double arg = (j[m] * j[n]) / S;
        const float v = (float)(2.0L * ::j0l((long double)arg) / (aj1[m] * aj1[n] * (long double)S));
        Tp[(size_t)m * ld + n] = v;
        Tp[(size_t)n * ld + m] = v;
      }
  };
  std::vector<std::thread> pool;
  for (int i = 1; i < nth; ++i) pool.emplace_back(rows, i);
  rows(0);
  for (auto& th : pool) th.join();
}

// ---- the per-device cache (as the CZT chirp tables: immutable, built on first use) -----------------
struct HkTable {
  float* T = nullptr;
  float* w = nullptr;
  double* zeros = nullptr;
  int ld = 0;
};
static std::mutex g_hk_mu;
static std::map<std::pair<int, int>, HkTable> g_hk;  // (device, N)

static int hk_ld(int N) { return (N + 3) & ~3; }

static int hk_table(int N, HkTable* out) {
  int dev = 0;
  THZ_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_hk_mu);
  const auto key = std::make_pair(dev, N);
  auto it = g_hk.find(key);
  if (it == g_hk.end()) {
    HkTable t;
    t.ld = hk_ld(N);
    std::vector<double> zeros;
    std::vector<float> w, T;
    hk_build(N, t.ld, &zeros, &w, &T);
    THZ_HIP_CHECK(hipMalloc(&t.T, T.size() * sizeof(float)));
    THZ_HIP_CHECK(hipMalloc(&t.w, w.size() * sizeof(float)));
    THZ_HIP_CHECK(hipMalloc(&t.zeros, zeros.size() * sizeof(double)));
    THZ_HIP_CHECK(hipMemcpy(t.T, T.data(), T.size() * sizeof(float), hipMemcpyHostToDevice));
    THZ_HIP_CHECK(hipMemcpy(t.w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    THZ_HIP_CHECK(hipMemcpy(t.zeros, zeros.data(), zeros.size() * sizeof(double), hipMemcpyHostToDevice));
    it = g_hk.emplace(key, t).first;
  }
  *out = it->second;
  return THZ_OK;
}

// ---- the host plan ------------------------------------------------------------------------------
struct HkPlan {
  int nt, rt, cb, S, kc, Mp;
  size_t pbytes;
};

static HkPlan hk_plan(int M, int K, long long ncc) {
  HkPlan p;
  p.nt = 2 * ncc <= 32 ? 1 : 2 * ncc <= 64 ? 2 : 4;
  p.rt = (M + HK_BM - 1) / HK_BM;
  p.cb = (int)((ncc + 16 * p.nt - 1) / (16 * p.nt));
  const long long tiles = (long long)p.rt * p.cb;
  const int want = (int)std::max(1LL, HK_TARGET / tiles);
  const int S = std::min(want, (K + HK_KMIN - 1) / HK_KMIN);
  p.kc = ((K + S - 1) / S + HK_BK - 1) / HK_BK * HK_BK;
  p.S = (K + p.kc - 1) / p.kc;
  p.Mp = (M + 3) & ~3;
  p.pbytes = align256((size_t)p.S * 2 * (size_t)ncc * p.Mp * sizeof(float));
  return p;
}

constexpr long long HK_MAX_COLUMNS = 1LL << 20;  // complex columns Z B C of one call (grid.y and 32-bit indices)

static int hk_check(const char* who, const thz_hankel_desc* d, bool need_z) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->N < 1 || d->N > HK_MAX_N) return fail(THZ_E_ARG, "%s: N = %d outside [1, %d]", who, d->N, HK_MAX_N);
  if (d->keep < 1 || d->keep > d->N) return fail(THZ_E_ARG, "%s: keep = %d outside [1, N = %d]", who, d->keep, d->N);
  if (d->Z < 1 || d->B < 1 || d->C < 1) return fail(THZ_E_ARG, "%s: bad shape Z=%d B=%d C=%d", who, d->Z, d->B, d->C);
  if (!(d->r_max > 0.0)) return fail(THZ_E_ARG, "%s: r_max = %g is not positive", who, d->r_max);
  if (!d->wavelengths) return fail(THZ_E_ARG, "%s: null wavelengths", who);
  if (d->C > THZ_MAX_WAVELENGTHS) return fail(THZ_E_UNSUPPORTED, "%s: C=%d > %d", who, d->C, THZ_MAX_WAVELENGTHS);
  for (int c = 0; c < d->C; ++c)
    if (!(d->wavelengths[c] > 0.0f)) return fail(THZ_E_ARG, "%s: wavelength[%d] = %g is not positive", who, c, (double)d->wavelengths[c]);
  if (need_z && !d->z && !d->z_dev) return fail(THZ_E_ARG, "%s: null z and z_dev", who);
  if (d->Z > THZ_MAX_Z) return fail(THZ_E_UNSUPPORTED, "%s: Z=%d > %d", who, d->Z, THZ_MAX_Z);
  if ((long long)d->Z * d->B * d->C > HK_MAX_COLUMNS)
    return fail(THZ_E_UNSUPPORTED, "%s: Z B C = %lld columns > %lld", who, (long long)d->Z * d->B * d->C, HK_MAX_COLUMNS);
  if (d->z_dev && misaligned(d->z_dev, sizeof(float))) return fail(THZ_E_ARG, "%s: z_dev not 4-byte aligned", who);
  return THZ_OK;
}

struct HkLayout {
  HkPlan narrow, wide;  // the B C-column product and the Z B C-column product
  size_t h_off, f_off, p_off, total;
};

static HkLayout hk_layout(const thz_hankel_desc* d, bool adjoint) {
  HkLayout L;
  const long long bc = (long long)d->B * d->C;
  L.narrow = hk_plan(d->N, d->N, bc);
  L.wide = adjoint ? hk_plan(d->N, d->keep, bc * d->Z) : hk_plan(d->keep, d->N, bc * d->Z);
  L.h_off = 0;
  L.f_off = align256((size_t)d->Z * d->C * d->N * sizeof(float2));
  L.p_off = L.f_off + align256((size_t)bc * d->N * sizeof(float2));
  L.total = L.p_off + std::max(L.narrow.pbytes, L.wide.pbytes);
  return L;
}

static int hk_tf(const thz_hankel_desc* d, const HkTable& t, float2* H, hipStream_t s) {
  HkTf a{};
  a.Z = d->Z; a.C = d->C; a.N = d->N;
  a.r_max = d->r_max;
  a.zeros = t.zeros;
  a.z_dev = d->z_dev;
  a.H = H;
  for (int i = 0; i < d->Z; ++i) a.z[i] = d->z_dev ? 0.0f : d->z[i];
  for (int c = 0; c < d->C; ++c) a.lam[c] = d->wavelengths[c];
  const long long total = (long long)d->Z * d->C * d->N;
  int blocks = 0;
  if (int e = stream_grid((total + HK_THREADS - 1) / HK_THREADS, &blocks)) return e;
  KernelTimer kt("hankel_tf", s);
  hipLaunchKernelGGL(hankel_tf_kernel, dim3((unsigned)blocks), dim3(HK_THREADS), 0, s, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

template <bool HMODE>
static void hk_launch_gemm(const HkPlan& p, const HkGemm& a, hipStream_t s) {
  const dim3 grid((unsigned)p.rt, (unsigned)p.cb, (unsigned)p.S), block(HK_THREADS);
  if (p.nt == 1) hipLaunchKernelGGL((hankel_gemm_kernel<1, HMODE>), grid, block, 0, s, a);
  else if (p.nt == 2) hipLaunchKernelGGL((hankel_gemm_kernel<2, HMODE>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((hankel_gemm_kernel<4, HMODE>), grid, block, 0, s, a);
}

// One product and its finish.  H: with `zsum` the finish's conj(H) and plane sum, otherwise the loader's H.
static int hk_product(const HkPlan& p, const HkTable& t, int M, int K, int ncc, int pre, int post, const float2* X,
                      const float2* H, bool zsum, const thz_hankel_desc* d, float* P, float2* out, hipStream_t s) {
  HkGemm a{};
  a.T = t.T; a.w = t.w; a.X = X; a.H = zsum ? nullptr : H; a.P = P;
  a.ldT = t.ld; a.M = M; a.K = K; a.ncc = ncc; a.Mp = p.Mp; a.kc = p.kc; a.pre = pre;
  a.BC = d->B * d->C; a.C = d->C;
  {
    KernelTimer kt("hankel_gemm", s);
    if (a.H) hk_launch_gemm<true>(p, a, s);
    else hk_launch_gemm<false>(p, a, s);
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  HkFinish f{};
  f.P = P; f.w = t.w; f.H = zsum ? H : nullptr; f.out = out;
  f.S = p.S; f.ncc = ncc; f.Mp = p.Mp; f.M = M; f.post = post; f.Z = d->Z; f.BC = a.BC; f.C = d->C;
  const long long total = (long long)(zsum ? a.BC : ncc) * M;
  int blocks = 0;
  if (int e = stream_grid((total + HK_THREADS - 1) / HK_THREADS, &blocks)) return e;
  KernelTimer kt("hankel_finish", s);
  if (zsum) hipLaunchKernelGGL(hankel_finish_kernel<true>, dim3((unsigned)blocks), dim3(HK_THREADS), 0, s, f);
  else hipLaunchKernelGGL(hankel_finish_kernel<false>, dim3((unsigned)blocks), dim3(HK_THREADS), 0, s, f);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

static int hk_run(const char* who, const thz_hankel_desc* d, const void* in, void* out, void* workspace, size_t bytes,
                  thz_stream_t stream, bool adjoint) {
  if (int e = hk_check(who, d, true)) return e;
  if (int e = check_arrays(who, {in, out}, sizeof(float2))) return e;
  const HkLayout L = hk_layout(d, adjoint);
  if (int e = check_workspace(workspace, bytes, L.total)) return e;
  if (misaligned(workspace, 256)) return fail(THZ_E_ARG, "%s: workspace not 256-byte aligned", who);
  HkTable t;
  if (int e = hk_table(d->N, &t)) return e;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float2* H = (float2*)(ws + L.h_off);
  float2* F = (float2*)(ws + L.f_off);
  float* P = (float*)(ws + L.p_off);
  const int bc = d->B * d->C, N = d->N;
  if (int e = hk_tf(d, t, H, s)) return e;
  if (!adjoint) {
    if (int e = hk_product(L.narrow, t, N, N, bc, HK_W, HK_ONE, (const float2*)in, nullptr, false, d, P, F, s)) return e;
    return hk_product(L.wide, t, d->keep, N, d->Z * bc, HK_ONE, HK_WINV, F, H, false, d, P, (float2*)out, s);
  }
  if (int e = hk_product(L.wide, t, N, d->keep, d->Z * bc, HK_WINV, HK_ONE, (const float2*)in, H, true, d, P, F, s)) return e;
  return hk_product(L.narrow, t, N, N, bc, HK_ONE, HK_W, F, nullptr, false, d, P, (float2*)out, s);
}

}  // namespace thz

using namespace thz;

extern "C" int thz_hankel_workspace_size(const thz_hankel_desc* d, size_t* bytes) {
  const char* who = "thz_hankel_workspace_size";
  if (!bytes) return fail(THZ_E_ARG, "%s: null bytes", who);
  if (int e = hk_check(who, d, false)) return e;
  // one size serves the forward and the adjoint
  *bytes = std::max(hk_layout(d, false).total, hk_layout(d, true).total);
  return THZ_OK;
}

extern "C" int thz_hankel_forward(const thz_hankel_desc* d, const void* profile, void* out, void* workspace,
                                  size_t workspace_bytes, thz_stream_t stream) {
  return hk_run("thz_hankel_forward", d, profile, out, workspace, workspace_bytes, stream, false);
}

extern "C" int thz_hankel_adjoint(const thz_hankel_desc* d, const void* grad_out, void* grad_profile, void* workspace,
                                  size_t workspace_bytes, thz_stream_t stream) {
  return hk_run("thz_hankel_adjoint", d, grad_out, grad_profile, workspace, workspace_bytes, stream, true);
}

extern "C" int thz_hankel_table_host(int N, float* out_T, float* out_w, double* out_zeros) {
  const char* who = "thz_hankel_table_host";
  if (N < 1 || N > HK_MAX_N) return fail(THZ_E_ARG, "%s: N = %d outside [1, %d]", who, N, HK_MAX_N);
  if (!out_T || !out_w || !out_zeros) return fail(THZ_E_ARG, "%s: null pointer", who);
  std::vector<double> zeros;
  std::vector<float> w, T;
  hk_build(N, N, &zeros, &w, &T);
  std::copy(T.begin(), T.end(), out_T);
  std::copy(w.begin(), w.end(), out_w);
  std::copy(zeros.begin(), zeros.end(), out_zeros);
  return THZ_OK;
}

extern "C" int thz_hankel_table(int N, float* out_T, float* out_w, double* out_zeros, thz_stream_t stream) {
  const char* who = "thz_hankel_table";
  if (N < 1 || N > HK_MAX_N) return fail(THZ_E_ARG, "%s: N = %d outside [1, %d]", who, N, HK_MAX_N);
  if (int e = check_arrays(who, {out_T, out_w}, sizeof(float))) return e;
  if (int e = check_arrays(who, {out_zeros}, sizeof(double))) return e;
  HkTable t;
  if (int e = hk_table(N, &t)) return e;
  hipStream_t s = (hipStream_t)stream;
  THZ_HIP_CHECK(hipMemcpy2DAsync(out_T, (size_t)N * sizeof(float), t.T, (size_t)t.ld * sizeof(float), (size_t)N * sizeof(float),
                                 (size_t)N, hipMemcpyDeviceToDevice, s));
  THZ_HIP_CHECK(hipMemcpyAsync(out_w, t.w, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s));
  THZ_HIP_CHECK(hipMemcpyAsync(out_zeros, t.zeros, (size_t)(N + 1) * sizeof(double), hipMemcpyDeviceToDevice, s));
  return THZ_OK;
}

extern "C" int thz_hankel_transfer_function(const thz_hankel_desc* d, void* out, thz_stream_t stream) {
  const char* who = "thz_hankel_transfer_function";
  if (int e = hk_check(who, d, true)) return e;
  if (int e = check_arrays(who, {out}, sizeof(float2))) return e;
  HkTable t;
  if (int e = hk_table(d->N, &t)) return e;
  return hk_tf(d, t, (float2*)out, (hipStream_t)stream);
}
