// Time-domain THz pulses: broadband synthesis and per-pixel pulse maps (include/thzdoe.h: thz_pulse_*; pulse.py;
// DESIGN §39).  Not part of the reference.  The per-frequency phasors U[b, c, p] of a field become the analytic signal
// E[b, j, p] = sum_c Phi[j, c] U[b, c, p] at T time samples, and this unit is that product and its adjoint on the fp32
// matrix cores (v_mfma_f32_32x32x2_f32: A 32 x 2, B 2 x 32, lane (l, h) = (lane % 32, lane / 32) holds A[l][h] and
// B[h][l], accumulator v of that lane is D[8 (v / 4) + 4 h + v % 4][l]).
//
//   real form    k = 2 c + part over [Re U_c, Im U_c]: one MFMA contracts the k pair of one channel, the lane half h is
//                the part.  Rows Re E_j take A = (Phi_r, -Phi_i), rows Im E_j take A = (Phi_i, Phi_r), so a wave holds
//                two accumulator tiles of the same 32 samples x 32 pixels and |E_j|^2 forms in a lane.  No K tail: an
//                odd C is C MFMAs per tile.
//   split        A workgroup of four waves owns 128 consecutive pixels of one batch entry, a wave 32 of them; a tile
//                never crosses a batch entry and the last one is predicated.  The B operand of a wave -- its pixels'
//                2 C reals -- is loaded once into C registers per lane (lane (p, h) reads part h of pixel p: a wave's
//                load covers 256 contiguous bytes of a channel row) and stays there for every time tile: the field is
//                read from memory exactly once whatever T is, and it never needs LDS.
//   table        What goes through LDS is the small operand that all four waves share: the 32 samples x C channels of
//                a time tile, staged as complex sA[c][j] at a row stride of 33 complex numbers, rows c >= C and samples
//                j >= T zero.  The staging writes (consecutive lanes, consecutive c) step 66 floats = 2 banks, the
//                first product reads row c at consecutive j (lane l = j, both halves the same address), and the second
//                product reads column j at consecutive c (lane l = c): every access is an 8-byte one that touches
//                each bank pair once.  The next tile's global loads are in flight while the current one is multiplied.
//                A ds_read feeds two (first product) or four (second product) 64-cycle MFMAs, so 16-byte LDS reads
//                would buy nothing here.
//   synthesize   stores the two accumulators as complex numbers: row j of a tile is 32 consecutive pixels on 32
//                consecutive lanes, 256 contiguous bytes.  With few pixels the time tiles are dealt to grid.y.
//   maps         the epilogue of each time tile updates a lane's running W, M1, M2 (fp64, moments about the middle of
//                the time window) and (peak, j*) over its 16 rows in ascending j; after the last tile the two lane
//                halves are merged (h = 0 first) and lane (p, 0) writes the five maps.  The time-resolved field
//                never reaches memory.  Summation order: a lane's rows 8 a + 4 h + b of tile 0 in ascending (a, b),
//                then tile 1, ...; then half 0 + half 1.
//   second product   G[j, p] -> Ubar[c, p] = sum_j conj(Phi[j, c]) G[j, p]: accumulator v of lane (p, h) holds row
//                8 a + 4 h + b of a 32 x 32 tile, which is exactly the B operand of the MFMA that contracts the row pair
//                {8 a + b, 8 a + 4 + b}; the A operand Phi[j, c] comes from the same staged tile read by column.  Rows
//                are channels (32 per accumulator pair, Re and Im apart), so with C < 32 the rows above C multiply
//                zeros: accepted.  pulse_adjoint loads G from memory straight into that layout (a row is 256 contiguous
//                bytes); pulse_maps_backward recomputes the E tile, scales it in registers by 2 a_j from the saved
//                maps and the upstream gradients, and hands the accumulators over: E never reaches memory.
// No atomics, no workspace: every call gives the same bits, and a batch entry's bits do not depend on B.  fp contraction
// is off; the products are explicit MFMA.
#include <math.h>

#include <algorithm>

#include "thz_common.hpp"
#include "thz_launch.hpp"

#pragma clang fp contract(off)

namespace thz {

constexpr int PL_THREADS = 256;
constexpr int PL_PIX = 128;     // pixels of a workgroup (32 per wave)
constexpr int PL_TT = 32;       // samples of a time tile
constexpr int PL_LD = PL_TT + 1;  // row stride of the staged table tile, complex numbers
constexpr int PL_MAX_T = 4096;
constexpr long long PL_MAX_PIX = 2147483647LL;
constexpr int PL_FILL = 1024;   // synthesize: below this many workgroups the time tiles are dealt to grid.y

enum { PL_SYNTH = 0, PL_MAPS = 1, PL_MAPS_BWD = 2 };

typedef float pl_acc __attribute__((ext_vector_type(16)));

__device__ __forceinline__ pl_acc pl_zero() {
  pl_acc a;
#pragma unroll
  for (int v = 0; v < 16; ++v) a[v] = 0.0f;
  return a;
}

__device__ __forceinline__ pl_acc pl_mfma(float a, float b, pl_acc c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#else
  return c;  // the host pass compiles no MFMA
#endif
}

struct PlArgs {
  const float2* U;      // [B][C][HW]       the field (synthesize, maps, maps backward)
  const float2* table;  // [T][C]
  const float* times;   // [T]
  const float* dt;      // [T]
  float2* E;            // [B][T][HW]       synthesize
  const float2* G;      // [B][T][HW]       adjoint
  float* maps;          // [B][5][HW]       written by maps, read by its backward
  const float* gmaps;   // [B][5][HW]
  float2* gU;           // [B][C][HW]       adjoint, maps backward
  long long HW, tiles;  // pixels and workgroups per batch entry
  int C, T, tt_per_y;
};

// the table tile at sample j0 through registers into sA[c][j]; CP rows, those at and above C zero
template <int CP>
struct PlStage {
  float2 r[CP / 8];
  float rt, rdt;
  __device__ __forceinline__ void fetch(const PlArgs& a, int j0, int t, bool with_times) {
#pragma unroll
    for (int i = 0; i < CP / 8; ++i) {
      const int e = t + PL_THREADS * i, c = e % CP, j = j0 + e / CP;
      r[i] = (c < a.C && j < a.T) ? a.table[(size_t)j * a.C + c] : make_float2(0.f, 0.f);
    }
    if (with_times && t < PL_TT) {
      const bool in = j0 + t < a.T;
      rt = in ? a.times[j0 + t] : 0.f;
      rdt = in ? a.dt[j0 + t] : 0.f;
    }
  }
  __device__ __forceinline__ void put(float2* sA, float* sT, float* sDt, int t, bool with_times) const {
#pragma unroll
    for (int i = 0; i < CP / 8; ++i) {
      const int e = t + PL_THREADS * i;
      sA[(e % CP) * PL_LD + e / CP] = r[i];
    }
    if (with_times && t < PL_TT) {
      sT[t] = rt;
      sDt[t] = rdt;
    }
  }
};

// E tile = Phi tile x U: lane (j, h) takes (Phi_r, -Phi_i)[h] for the Re rows and (Phi_i, Phi_r)[h] for the Im rows
template <int CR>
__device__ __forceinline__ void pl_first(const float2* sA, const float (&u)[CR], int C, int li, int lh, pl_acc& ere,
                                         pl_acc& eim) {
#pragma unroll
  for (int c = 0; c < CR; ++c) {
    if (c < C) {  // uniform; a break would keep the loop, and u, from being unrolled into registers
      const float2 f = sA[c * PL_LD + li];
      ere = pl_mfma(lh ? -f.y : f.x, u[c], ere);
      eim = pl_mfma(lh ? f.x : f.y, u[c], eim);
    }
  }
}

// Ubar[c, p] += sum_j conj(Phi[j, c]) G[j, p] over the tile's 32 samples: MFMA v contracts the rows {8 a + b, 8 a + 4 + b}
// that accumulator v = 4 a + b of the two lane halves holds; lane (c, h) reads Phi[8 a + 4 h + b][32 nb + c]
template <int NB>
__device__ __forceinline__ void pl_second(const float2* sA, int C, int li, int lh, const pl_acc& gr, const pl_acc& gi,
                                          pl_acc (&ore)[NB], pl_acc (&oim)[NB]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (32 * nb < C)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float2 f = sA[(32 * nb + li) * PL_LD + 8 * (v / 4) + 4 * lh + v % 4];
      ore[nb] = pl_mfma(f.x, gr[v], ore[nb]);
      ore[nb] = pl_mfma(f.y, gi[v], ore[nb]);
      oim[nb] = pl_mfma(f.x, gi[v], oim[nb]);
      oim[nb] = pl_mfma(-f.y, gr[v], oim[nb]);
    }
  }
}

// accumulator v of lane (p, h) is channel 32 nb + 8 a + 4 h + b of pixel p: a row is 256 contiguous bytes
template <int NB>
__device__ __forceinline__ void pl_store_grad(float2* gU, int C, long long HW, long long p, bool live, int lh,
                                              const pl_acc (&ore)[NB], const pl_acc (&oim)[NB]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int c = 32 * nb + 8 * (v / 4) + 4 * lh + v % 4;
      if (live && c < C) gU[(size_t)c * HW + p] = make_float2(ore[nb][v], oim[nb][v]);
    }
}

template <int CR, int MODE>
__global__ void __launch_bounds__(PL_THREADS) pulse_forward_kernel(PlArgs a) {
  constexpr int CP = CR < 32 ? 32 : CR;
  constexpr int NB = CP / 32;
  constexpr bool TIMES = MODE != PL_SYNTH;
  __shared__ float2 sA[CP * PL_LD];
  __shared__ float sT[PL_TT], sDt[PL_TT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const long long b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const long long p = tile * PL_PIX + wave * 32 + li;
  const bool live = p < a.HW;
  const int C = a.C, T = a.T;

  // the wave's B operand: part lh of every channel of pixel p
  const float* Uf = reinterpret_cast<const float*>(a.U + (size_t)b * C * a.HW);
  float u[CR];
#pragma unroll
  for (int c = 0; c < CR; ++c) u[c] = (live && c < C) ? Uf[2 * ((size_t)c * a.HW + p) + lh] : 0.f;

  // maps: running sums of this lane's rows; maps backward: the pixel's coefficients of a_j
  double sW = 0.0, sM1 = 0.0, sM2 = 0.0, tc = 0.0;
  float pk = -1.0f;
  int jstar = 0x7fffffff;
  double cW = 0.0, c1 = 0.0, c2 = 0.0, s2 = 0.0, tm = 0.0;
  float tpk = 0.f, gpk = 0.f;
  pl_acc ore[NB], oim[NB];
  (void)sW; (void)sM1; (void)sM2; (void)tc; (void)pk; (void)jstar;
  (void)cW; (void)c1; (void)c2; (void)s2; (void)tm; (void)tpk; (void)gpk; (void)ore; (void)oim;
  if constexpr (MODE == PL_MAPS) tc = 0.5 * ((double)a.times[0] + (double)a.times[T - 1]);
  if constexpr (MODE == PL_MAPS_BWD) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) ore[nb] = pl_zero(), oim[nb] = pl_zero();
    if (live) {
      const float* m = a.maps + (size_t)b * 5 * a.HW + p;
      const float* g = a.gmaps + (size_t)b * 5 * a.HW + p;
      const double W = (double)m[0], trms = (double)m[4 * a.HW];
      tpk = m[2 * a.HW];
      tm = (double)m[3 * a.HW];
      cW = (double)g[0];
      gpk = g[a.HW];
      if (W > 0.0) {
        c1 = (double)g[3 * a.HW] / W;
        if (trms > 0.0) c2 = (double)g[4 * a.HW] / (2.0 * trms * W);
      }
      s2 = trms * trms;
    }
  }

  const int ntiles = (T + PL_TT - 1) / PL_TT;
  int tt0 = 0, tt1 = ntiles;
  if constexpr (MODE == PL_SYNTH) {
    tt0 = blockIdx.y * a.tt_per_y;
    tt1 = min(ntiles, tt0 + a.tt_per_y);
  }
  PlStage<CP> st;
  if (tt0 < tt1) st.fetch(a, tt0 * PL_TT, t, TIMES);
  for (int tt = tt0; tt < tt1; ++tt) {
    const int j0 = tt * PL_TT;
    st.put(sA, sT, sDt, t, TIMES);
    __syncthreads();
    if (tt + 1 < tt1) st.fetch(a, j0 + PL_TT, t, TIMES);
    pl_acc ere = pl_zero(), eim = pl_zero();
    pl_first<CR>(sA, u, C, li, lh, ere, eim);

    if constexpr (MODE == PL_SYNTH) {
      float2* E = a.E + ((size_t)b * T + j0) * a.HW + p;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int r = 8 * (v / 4) + 4 * lh + v % 4;
        if (live && j0 + r < T) E[(size_t)r * a.HW] = make_float2(ere[v], eim[v]);
      }
    } else if constexpr (MODE == PL_MAPS) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int r = 8 * (v / 4) + 4 * lh + v % 4;
        if (j0 + r < T) {
          const float I = ere[v] * ere[v] + eim[v] * eim[v];
          const double w = (double)I * (double)sDt[r], tau = (double)sT[r] - tc;
          sW += w;
          sM1 += tau * w;
          sM2 += tau * tau * w;
          if (I > pk) pk = I, jstar = j0 + r;
        }
      }
    } else {
      // G = 2 a_j E in place, then the second product
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int r = 8 * (v / 4) + 4 * lh + v % 4;
        const float tj = sT[r];
        const double d = (double)tj - tm;
        double aj = (double)sDt[r] * (cW + c1 * d + c2 * (d * d - s2));
        if (j0 + r < T && tj == tpk) aj += (double)gpk;
        const float s = (float)(2.0 * aj);
        ere[v] *= s;
        eim[v] *= s;
      }
      pl_second<NB>(sA, C, li, lh, ere, eim, ore, oim);
    }
    __syncthreads();
  }

  if constexpr (MODE == PL_MAPS) {
    // half 1 into half 0, then the pixel's five maps
    const double oW = __shfl_xor(sW, 32), oM1 = __shfl_xor(sM1, 32), oM2 = __shfl_xor(sM2, 32);
    const float opk = __shfl_xor(pk, 32);
    const int oj = __shfl_xor(jstar, 32);
    if (lh == 0 && live) {
      const double W = sW + oW, M1 = sM1 + oM1, M2 = sM2 + oM2;
      if (opk > pk || (opk == pk && oj < jstar)) pk = opk, jstar = oj;
      float tmean = 0.f, trms = 0.f;
      if (W > 0.0) {
        const double m1 = M1 / W, var = M2 / W - m1 * m1;
        tmean = (float)(tc + m1);
        trms = var > 0.0 ? (float)sqrt(var) : 0.f;
      }
      float* m = a.maps + (size_t)b * 5 * a.HW + p;
      m[0] = (float)W;
      m[a.HW] = pk;
      m[2 * a.HW] = a.times[jstar < T ? jstar : 0];  // a NaN intensity never wins the comparison
      m[3 * a.HW] = tmean;
      m[4 * a.HW] = trms;
    }
  }
  if constexpr (MODE == PL_MAPS_BWD) pl_store_grad<NB>(a.gU + (size_t)b * C * a.HW, C, a.HW, p, live, lh, ore, oim);
}

template <int NB>
__global__ void __launch_bounds__(PL_THREADS) pulse_adjoint_kernel(PlArgs a) {
  constexpr int CP = 32 * NB;
  __shared__ float2 sA[CP * PL_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const long long b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const long long p = tile * PL_PIX + wave * 32 + li;
  const bool live = p < a.HW;
  const int C = a.C, T = a.T;
  const float2* G = a.G + (size_t)b * T * a.HW + p;

  // rows 8 a + 4 lh + b of the tile at j0, the layout of an accumulator
  float2 g[16], gn[16];
  auto fetch = [&](int j0, float2* o) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int j = j0 + 8 * (v / 4) + 4 * lh + v % 4;
      o[v] = (live && j < T) ? G[(size_t)j * a.HW] : make_float2(0.f, 0.f);
    }
  };
  pl_acc ore[NB], oim[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) ore[nb] = pl_zero(), oim[nb] = pl_zero();

  const int ntiles = (T + PL_TT - 1) / PL_TT;
  PlStage<CP> st;
  st.fetch(a, 0, t, false);
  fetch(0, g);
  for (int tt = 0; tt < ntiles; ++tt) {
    const int j0 = tt * PL_TT;
    st.put(sA, nullptr, nullptr, t, false);
    __syncthreads();
    const bool more = tt + 1 < ntiles;
    if (more) {
      st.fetch(a, j0 + PL_TT, t, false);
      fetch(j0 + PL_TT, gn);
    }
    pl_acc gr, gi;
#pragma unroll
    for (int v = 0; v < 16; ++v) gr[v] = g[v].x, gi[v] = g[v].y;
    pl_second<NB>(sA, C, li, lh, gr, gi, ore, oim);
    __syncthreads();
    if (more) {
#pragma unroll
      for (int v = 0; v < 16; ++v) g[v] = gn[v];
    }
  }
  pl_store_grad<NB>(a.gU + (size_t)b * C * a.HW, C, a.HW, p, live, lh, ore, oim);
}

// ---- host checks and launches ---------------------------------------------------------------------
static int pl_check(const char* who, const thz_pulse_desc* d) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->B < 1 || d->H < 1 || d->W < 1) return fail(THZ_E_ARG, "%s: bad shape B=%d H=%d W=%d", who, d->B, d->H, d->W);
  if (d->C < 1 || d->C > THZ_MAX_WAVELENGTHS)
    return fail(THZ_E_UNSUPPORTED, "%s: C = %d outside [1, %d]", who, d->C, THZ_MAX_WAVELENGTHS);
  if (d->T < 1 || d->T > PL_MAX_T) return fail(THZ_E_UNSUPPORTED, "%s: T = %d outside [1, %d]", who, d->T, PL_MAX_T);
  const long long HW = (long long)d->H * d->W;
  if (HW > PL_MAX_PIX) return fail(THZ_E_UNSUPPORTED, "%s: H W = %lld above 2^31 - 1", who, HW);
  if ((long long)d->B * ((HW + PL_PIX - 1) / PL_PIX) > PL_MAX_PIX)
    return fail(THZ_E_UNSUPPORTED, "%s: B x ceil(H W / %d) = %lld workgroups above 2^31 - 1", who, PL_PIX,
                (long long)d->B * ((HW + PL_PIX - 1) / PL_PIX));
  return THZ_OK;
}

static PlArgs pl_args(const thz_pulse_desc* d, const void* table) {
  PlArgs a{};
  a.table = (const float2*)table;
  a.HW = (long long)d->H * d->W;
  a.tiles = (a.HW + PL_PIX - 1) / PL_PIX;
  a.C = d->C;
  a.T = d->T;
  a.tt_per_y = (d->T + PL_TT - 1) / PL_TT;
  return a;
}

template <int MODE>
static void pl_launch_forward(const PlArgs& a, dim3 grid, hipStream_t s) {
  if (a.C <= 8)
    hipLaunchKernelGGL((pulse_forward_kernel<8, MODE>), grid, dim3(PL_THREADS), 0, s, a);
  else if (a.C <= 32)
    hipLaunchKernelGGL((pulse_forward_kernel<32, MODE>), grid, dim3(PL_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((pulse_forward_kernel<64, MODE>), grid, dim3(PL_THREADS), 0, s, a);
}

}  // namespace thz

using namespace thz;

extern "C" int thz_pulse_synthesize(const thz_pulse_desc* d, const void* field, const void* table, void* out,
                                    thz_stream_t stream) {
  const char* who = "thz_pulse_synthesize";
  if (int e = pl_check(who, d)) return e;
  if (int e = check_arrays(who, {field, table, out}, sizeof(float2))) return e;
  PlArgs a = pl_args(d, table);
  a.U = (const float2*)field;
  a.E = (float2*)out;
  // too few pixels to fill the device: the time tiles go to grid.y, each a run of tt_per_y tiles
  const long long wgs = d->B * a.tiles;
  const int ntiles = a.tt_per_y;
  int ny = 1;
  if (wgs < PL_FILL) ny = (int)std::min<long long>(ntiles, (PL_FILL + wgs - 1) / wgs);
  a.tt_per_y = (ntiles + ny - 1) / ny;
  ny = (ntiles + a.tt_per_y - 1) / a.tt_per_y;
  hipStream_t s = (hipStream_t)stream;
  KernelTimer kt("pulse_synthesize", s);
  pl_launch_forward<PL_SYNTH>(a, dim3((unsigned)wgs, (unsigned)ny), s);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_pulse_adjoint(const thz_pulse_desc* d, const void* grad_out, const void* table, void* grad_field,
                                 thz_stream_t stream) {
  const char* who = "thz_pulse_adjoint";
  if (int e = pl_check(who, d)) return e;
  if (int e = check_arrays(who, {grad_out, table, grad_field}, sizeof(float2))) return e;
  PlArgs a = pl_args(d, table);
  a.G = (const float2*)grad_out;
  a.gU = (float2*)grad_field;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(d->B * a.tiles));
  KernelTimer kt("pulse_adjoint", s);
  if (d->C <= 32)
    hipLaunchKernelGGL(pulse_adjoint_kernel<1>, grid, dim3(PL_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(pulse_adjoint_kernel<2>, grid, dim3(PL_THREADS), 0, s, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_pulse_maps(const thz_pulse_desc* d, const void* field, const void* table, const float* times,
                              const float* dt, float* maps, thz_stream_t stream) {
  const char* who = "thz_pulse_maps";
  if (int e = pl_check(who, d)) return e;
  if (int e = check_arrays(who, {field, table}, sizeof(float2))) return e;
  if (int e = check_arrays(who, {times, dt, maps}, sizeof(float))) return e;
  PlArgs a = pl_args(d, table);
  a.U = (const float2*)field;
  a.times = times;
  a.dt = dt;
  a.maps = maps;
  hipStream_t s = (hipStream_t)stream;
  KernelTimer kt("pulse_maps", s);
  pl_launch_forward<PL_MAPS>(a, dim3((unsigned)(d->B * a.tiles)), s);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_pulse_maps_backward(const thz_pulse_desc* d, const void* field, const void* table, const float* times,
                                       const float* dt, const float* maps, const float* grad_maps, void* grad_field,
                                       thz_stream_t stream) {
  const char* who = "thz_pulse_maps_backward";
  if (int e = pl_check(who, d)) return e;
  if (int e = check_arrays(who, {field, table, grad_field}, sizeof(float2))) return e;
  if (int e = check_arrays(who, {times, dt, maps, grad_maps}, sizeof(float))) return e;
  PlArgs a = pl_args(d, table);
  a.U = (const float2*)field;
  a.times = times;
  a.dt = dt;
  a.maps = const_cast<float*>(maps);
  a.gmaps = grad_maps;
  a.gU = (float2*)grad_field;
  hipStream_t s = (hipStream_t)stream;
  KernelTimer kt("pulse_maps_bwd", s);
  pl_launch_forward<PL_MAPS_BWD>(a, dim3((unsigned)(d->B * a.tiles)), s);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
