// The z-x slice of the Rayleigh-Sommerfeld convolution (Props/RSC_Prop.py), forward and adjoint, for
// gfx950.  The planes (thz_rsc_forward) run on the ASM pipeline in thz_asm.hip; the slice shares
// with it the shape rules (rsc_shape) and the host toolkit (thz_launch.hpp), no kernel or layout.
#include <algorithm>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_launch.hpp"

namespace thz {

// ---------------------------------------------------------------------------------------------
// RSC / VRS z-x slice (thz_rsc_slice_forward): output row p of every plane of a z-sweep.  With
// K_{z,c}[a][j] = RS_{z,c}(x[a], y[j]) on the doubled grid, the 2-D circular convolution at output
// row H + p is a sum of H one-dimensional ones (it never wraps: 1 <= H + p - i <= Ph - 1):
//   out[k,b,c,q] = dx dy IFFT_Pw( sum_{i<H} FFT_Pw(in[b,c,i,:] padded)[m] FFT_Pw(K_{z_k,c}[H+p-i][:])[m] )[W+q]
//   rsc_slice_rows : Uh[u][c][i][:] = FFT_Pw of the zero-padded input rows, once per call (VRS: Ex, Ey
//                    once, and per plane of the chunk Ez, which carries z in its r)
//   rsc_slice_acc  : per (plane k, wavelength c, split s of the input rows, tile of b): kernel row ->
//                    FFT in LDS -> x Uh[b,c,i,:] -> partial sums in registers -> P[k][b C + c][s][:]
//   rsc_slice_line : per (k, b, c): the hs partials added in index order, inverse FFT, x dx dy / Pw,
//                    elements [W, Pw) -> out
// No column transform, no Ph x Pw table; every sum runs in a fixed order (no atomics).
// ---------------------------------------------------------------------------------------------
struct RscSliceArgs {
  int B, Bo, C, H, W, Ph, Pw;
  int vec, row;
  int nz, zoff;   // planes of this chunk, the first one's index into zv
  int hs, nbt;    // splits of the input rows, tiles of the Bo output planes per accumulate workgroup
  float dx, scale;
  float lam[THZ_MAX_WAVELENGTHS];
  float zv[THZ_MAX_Z];
};

// the Uh plane that holds output plane b of chunk plane kk: the field's planes, and for VRS Ez of kk
__device__ __forceinline__ int rss_uplane(const RscSliceArgs& a, int b, int kk) {
  return a.vec && b == 2 ? 2 + kk : b;
}

// Row spectra of the Uh planes [u0, u0 + gridDim.x / (C H)): one workgroup per (u, c, i).
template <int PN>
__global__ void __launch_bounds__(1024) rsc_slice_rows(const float2* __restrict__ in, float2* __restrict__ Uh,
                                                      FftPlan pw, RscSliceArgs a, int u0) {
  extern __shared__ float2 lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int i = blockIdx.x % a.H, c = (blockIdx.x / a.H) % a.C, u = u0 + blockIdx.x / (a.H * a.C);
  const bool ez = a.vec && u >= 2;
  // Ez = Ex x / r + Ey y / r on the unpadded grid (RowSrc), r with the z of chunk plane u - 2
  const float2* src = in + ((size_t)((ez ? 0 : u) * a.C + c) * a.H + i) * a.W;
  const float2* sy = in + ((size_t)(a.C + c) * a.H + i) * a.W;
  const float zr = ez ? a.zv[a.zoff + u - 2] : 0.f;
  const float xh = ez ? lin(-(float)a.H * a.dx / 2.0f, (float)a.H * a.dx / 2.0f, a.H, i) : 0.f;
  float2* dst = Uh + ((size_t)(u * a.C + c) * a.H + i) * a.Pw;
  auto load = [&](int j) {
    if (j >= a.W) return make_float2(0.f, 0.f);
    if (!ez) return src[j];
    return vrs_ez(src[j], sy[j], xh, lin(-(float)a.W * a.dx / 2.0f, (float)a.W * a.dx / 2.0f, a.W, j), zr);
  };
  if constexpr (PN > 0) {
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    auto ld = [&](int, int, int j) { return load(j); };
    auto sv = [&](int, int, int j, float2 v) { dst[j] = v; };
    fft_pow2_run<false, PN, Geo<PN>::T, FFT_ROWS>(lds, twl, tid, ld, sv);
  } else {
    for (int j = tid; j < a.Pw; j += nt) lds[padx(j)] = load(j);
    __syncthreads();
    fft_lds<false>(lds, pw, tid, nt);
    for (int j = tid; j < a.Pw; j += nt) dst[j] = lds[padx(j)];
  }
}

// Where a lane's 16 partial sums per output plane live over the row loop.  The compile-time plans of
// Pw = 1024, 2048, 4096, 8192 (at most 512 lanes, 256 VGPRs each): in registers, for one to three
// planes (VRS's) per workgroup.  The runtime plan (its stage calls keep their own registers; up to 1024 lanes of
// 128 VGPRs) would spill them: there the sums live in the workgroup's own slab of P, each element
// read, added to and written by the one lane that owns it, one plane per workgroup.  Pw = 16384 runs
// the runtime plan here: its compile-time form spilled at 128 VGPRs with the sums in either place.
// The host's choice of instantiation, block, LDS and tile is one function: rss_acc_select.
constexpr int RSS_BT_MAX = 3;
__host__ __device__ constexpr bool rss_acc_compiled(int pn) {
  return pn == 1024 || pn == 2048 || pn == 4096 || pn == 8192;
}
template <int PN>
__host__ __device__ constexpr int rss_threads_max() { return PN > 0 ? PN / pow2_v(PN) : 1024; }

template <int PN, int BT>
__global__ void __launch_bounds__(rss_threads_max<PN>()) rsc_slice_acc(const float2* __restrict__ Uh,
                                                                      float2* __restrict__ P, FftPlan pw,
                                                                      RscSliceArgs a) {
  constexpr bool REG = PN > 0;
  static_assert(PN == 0 || rss_acc_compiled(PN), "compile-time plans: 1024 .. 8192");
  static_assert(BT >= 1 && BT <= (REG ? RSS_BT_MAX : 1), "the sums in P: one plane per workgroup");
  extern __shared__ float2 lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  int id = blockIdx.x;
  const int bt = id % a.nbt; id /= a.nbt;
  const int s = id % a.hs; id /= a.hs;
  const int c = id % a.C, kk = id / a.C;
  const float z = a.zv[a.zoff + kk];
  const float lam = a.lam[c];
  const float kw = 6.283185307179586f / lam;
  const RsPhase rph = rs_phase(lam, z);
  // the kernel's grid as rsc_k_rows forms it: dx on both axes
  const float xlo = -(float)a.Ph * a.dx / 2.0f, xhi = (float)a.Ph * a.dx / 2.0f;
  const float ylo = -(float)a.Pw * a.dx / 2.0f, yhi = (float)a.Pw * a.dx / 2.0f;
  const int i0 = (int)((long long)s * a.H / a.hs), i1 = (int)((long long)(s + 1) * a.H / a.hs);  // hs <= H: not empty
  const int b0 = bt * BT;
  const float2* urow[BT];  // a tile's planes past Bo read plane Bo - 1 and are not stored
  float2* prow[BT];
#pragma unroll
  for (int t = 0; t < BT; ++t) {
    const int b = min(b0 + t, a.Bo - 1);
    urow[t] = Uh + (size_t)(rss_uplane(a, b, kk) * a.C + c) * a.H * a.Pw;
    prow[t] = P + (((size_t)(kk * a.Bo + b) * a.C + c) * a.hs + s) * a.Pw;
  }
  float2 acc[BT][16];
#pragma unroll
  for (int t = 0; t < BT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = make_float2(0.f, 0.f);
  // element j of row i's kernel spectrum, slot q of this lane
  auto add = [&](int i, int q, int j, float2 v) {
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      const float2 w = cmul(v, urow[t][(size_t)i * a.Pw + j]);
      if constexpr (REG) acc[t][q] = cadd(acc[t][q], w);
      else prow[t][j] = i == i0 ? w : cadd(prow[t][j], w);
    }
  };
  if constexpr (PN > 0) {
    constexpr int TT = Geo<PN>::T;
    using SC = Pow2Sched<PN>;
    constexpr int RL = SC::radix(SC::nst(FFT_ROWS) - 1, FFT_ROWS);  // the last stage hands (m, r), r < RL
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    for (int i = i0; i < i1; ++i) {
      const float xi = lin(xlo, xhi, a.Ph, a.H + a.row - i);
      auto ld = [&](int, int, int j) { return rs_kernel(xi, lin(ylo, yhi, PN, j), z, kw, rph); };
      auto sv = [&](int m, int r, int j, float2 v) { add(i, m * RL + r, j, v); };
      fft_pow2_run<false, PN, TT, FFT_ROWS>(lds, twl, tid, ld, sv);
    }
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      if (b0 + t >= a.Bo) break;
      // the last stage's result slots in its own order: (m, r) -> j = tid + m T + r L, L = PN / RL
#pragma unroll
      for (int q = 0; q < 16; ++q) prow[t][tid + (q / RL) * TT + (q % RL) * (PN / RL)] = acc[t][q];
    }
  } else {
    for (int i = i0; i < i1; ++i) {
      const float xi = lin(xlo, xhi, a.Ph, a.H + a.row - i);
      __syncthreads();  // the previous row's reads of the image are done
      for (int j = tid; j < a.Pw; j += nt) lds[padx(j)] = rs_kernel(xi, lin(ylo, yhi, a.Pw, j), z, kw, rph);
      __syncthreads();
      fft_lds<false>(lds, pw, tid, nt);
      for (int j = tid; j < a.Pw; j += nt) add(i, 0, j, lds[padx(j)]);
    }
  }
}

// One workgroup per (kk, b, c) = blockIdx.x: sum of the hs partials, inverse transform, the window.
template <int PN>
__global__ void __launch_bounds__(1024) rsc_slice_line(const float2* __restrict__ P, float2* __restrict__ out,
                                                      FftPlan pw, RscSliceArgs a) {
  extern __shared__ float2 lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const float2* src = P + (size_t)blockIdx.x * a.hs * a.Pw;
  const int Wo = a.Pw - a.W;
  float2* dst = out + ((size_t)a.zoff * a.Bo * a.C + blockIdx.x) * Wo;
  auto load = [&](int j) {
    float2 v = src[j];
    for (int s = 1; s < a.hs; ++s) v = cadd(v, src[(size_t)s * a.Pw + j]);
    return v;
  };
  if constexpr (PN > 0) {
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    auto ld = [&](int, int, int j) { return load(j); };
    auto sv = [&](int, int, int j, float2 v) {
      if (j >= a.W) dst[j - a.W] = cscale(v, a.scale);
    };
    fft_pow2_run<true, PN, Geo<PN>::T, FFT_ROWS>(lds, twl, tid, ld, sv);
  } else {
    for (int j = tid; j < a.Pw; j += nt) lds[padx(j)] = load(j);
    __syncthreads();
    fft_lds<true>(lds, pw, tid, nt);
    for (int w = tid; w < Wo; w += nt) dst[w] = cscale(lds[padx(a.W + w)], a.scale);
  }
}

// ---------------------------------------------------------------------------------------------
// Adjoint of the RSC / VRS z-x slice (thz_rsc_slice_adjoint), the forward's three steps reversed:
//   rsc_slice_line_adj : Gh[k][b C + c][:] = dx dy / Pw FFT_Pw(g[k,b,c,:] placed at [W, Pw)), per (k, b, c)
//   rsc_slice_acc_adj  : per (c, input row i, tile of b): for every plane of the chunk the kernel row
//                        -> FFT in LDS -> conj x Gh[k,b,c,:], summed over the planes in index order
//                        -> S[b][c][i][:] (the first chunk stores, later chunks read, add and store);
//                        VRS's third plane keeps its product rows per plane, S[2 + k][c][i][:]
//   rsc_slice_rows_adj : inverse FFT of the S rows, elements [0, W) -> grad_in; VRS's Ez rows per
//                        chunk, x x/r_k and y/r_k, added into grad_in[0] / grad_in[1] by the owning lane
// The same kernel values, transforms and grids as the forward; every sum in a fixed order.
// ---------------------------------------------------------------------------------------------
template <int PN>
__global__ void __launch_bounds__(1024) rsc_slice_line_adj(const float2* __restrict__ g, float2* __restrict__ Gh,
                                                          FftPlan pw, RscSliceArgs a) {
  extern __shared__ float2 lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int Wo = a.Pw - a.W;
  const float2* src = g + ((size_t)a.zoff * a.Bo * a.C + blockIdx.x) * Wo;
  float2* dst = Gh + (size_t)blockIdx.x * a.Pw;
  auto load = [&](int j) { return j >= a.W ? src[j - a.W] : make_float2(0.f, 0.f); };
  if constexpr (PN > 0) {
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    auto ld = [&](int, int, int j) { return load(j); };
    auto sv = [&](int, int, int j, float2 v) { dst[j] = cscale(v, a.scale); };
    fft_pow2_run<false, PN, Geo<PN>::T, FFT_ROWS>(lds, twl, tid, ld, sv);
  } else {
    for (int j = tid; j < a.Pw; j += nt) lds[padx(j)] = load(j);
    __syncthreads();
    fft_lds<false>(lds, pw, tid, nt);
    for (int j = tid; j < a.Pw; j += nt) dst[j] = cscale(lds[padx(j)], a.scale);
  }
}

// One workgroup per (c, i, tile of b); the sums over the chunk's planes live where rsc_slice_acc
// holds its sums over the rows: in registers on the compile-time plans, in the workgroup's own S rows
// (each element owned by one lane) on the runtime plan.  rss_acc_select picks both kernels alike.
template <int PN, int BT>
__global__ void __launch_bounds__(rss_threads_max<PN>()) rsc_slice_acc_adj(const float2* __restrict__ Gh,
                                                                          float2* __restrict__ S, FftPlan pw,
                                                                          RscSliceArgs a) {
  constexpr bool REG = PN > 0;
  static_assert(PN == 0 || rss_acc_compiled(PN), "compile-time plans: 1024 .. 8192");
  static_assert(BT >= 1 && BT <= (REG ? RSS_BT_MAX : 1), "the sums in S: one plane per workgroup");
  extern __shared__ float2 lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  int id = blockIdx.x;
  const int bt = id % a.nbt; id /= a.nbt;
  const int i = id % a.H, c = id / a.H;
  const float lam = a.lam[c];
  const float kw = 6.283185307179586f / lam;
  const float xlo = -(float)a.Ph * a.dx / 2.0f, xhi = (float)a.Ph * a.dx / 2.0f;
  const float ylo = -(float)a.Pw * a.dx / 2.0f, yhi = (float)a.Pw * a.dx / 2.0f;
  const float xi = lin(xlo, xhi, a.Ph, a.H + a.row - i);
  const bool first = a.zoff == 0;  // the first chunk stores S
  const int b0 = bt * BT;
  const size_t prow = (size_t)a.H * a.Pw, off = ((size_t)c * a.H + i) * a.Pw;
  const float2* grow[BT];  // a tile's planes past Bo read plane Bo - 1 and are not stored
  float2* srow[BT];        // the summed row; VRS's third plane: its row of chunk plane 0
  bool ez[BT];
#pragma unroll
  for (int t = 0; t < BT; ++t) {
    const int b = min(b0 + t, a.Bo - 1);
    ez[t] = a.vec && b == 2;
    grow[t] = Gh + (size_t)(b * a.C + c) * a.Pw;
    srow[t] = S + (size_t)b * a.C * prow + off;
  }
  const size_t gstep = (size_t)a.Bo * a.C * a.Pw, estep = (size_t)a.C * prow;  // per chunk plane
  float2 acc[BT][16];
#pragma unroll
  for (int t = 0; t < BT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = make_float2(0.f, 0.f);
  // element j of chunk plane kk's conjugated kernel-row spectrum times the cotangent lines, slot q
  auto add = [&](int kk, int q, int j, float2 v) {
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      const float2 w = cmulc(grow[t][kk * gstep + j], v);
      if (ez[t]) srow[t][kk * estep + j] = w;
      else if constexpr (REG) acc[t][q] = cadd(acc[t][q], w);
      else srow[t][j] = (first && kk == 0) ? w : cadd(srow[t][j], w);
    }
  };
  if constexpr (PN > 0) {
    constexpr int TT = Geo<PN>::T;
    using SC = Pow2Sched<PN>;
    constexpr int RL = SC::radix(SC::nst(FFT_ROWS) - 1, FFT_ROWS);
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    for (int kk = 0; kk < a.nz; ++kk) {
      const float z = a.zv[a.zoff + kk];
      const RsPhase rph = rs_phase(lam, z);
      auto ld = [&](int, int, int j) { return rs_kernel(xi, lin(ylo, yhi, PN, j), z, kw, rph); };
      auto sv = [&](int m, int r, int j, float2 v) { add(kk, m * RL + r, j, v); };
      fft_pow2_run<false, PN, TT, FFT_ROWS>(lds, twl, tid, ld, sv);
    }
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      if (b0 + t >= a.Bo) break;
      if (ez[t]) continue;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = tid + (q / RL) * TT + (q % RL) * (PN / RL);
        srow[t][j] = first ? acc[t][q] : cadd(srow[t][j], acc[t][q]);
      }
    }
  } else {
    for (int kk = 0; kk < a.nz; ++kk) {
      const float z = a.zv[a.zoff + kk];
      const RsPhase rph = rs_phase(lam, z);
      __syncthreads();  // the previous plane's reads of the image are done
      for (int j = tid; j < a.Pw; j += nt) lds[padx(j)] = rs_kernel(xi, lin(ylo, yhi, a.Pw, j), z, kw, rph);
      __syncthreads();
      fft_lds<false>(lds, pw, tid, nt);
      for (int j = tid; j < a.Pw; j += nt) add(kk, 0, j, lds[padx(j)]);
    }
  }
}

// The adjoint of vrs_ez: what a cotangent e of Ez adds to those of Ex and Ey, rounded as vrs_ez rounds.
#pragma clang fp contract(off)
__device__ __forceinline__ void vrs_ez_adj(float2 e, float x, float y, float z, float2& gx, float2& gy) {
  const float r = sqrtf(x * x + y * y + z * z);
  gx = make_float2((e.x * x) / r, (e.y * x) / r);
  gy = make_float2((e.x * y) / r, (e.y * y) / r);
}
#pragma clang fp contract(on)

// EZ false: one workgroup per (plane u, c, i) of the summed S rows, after the last chunk: the inverse
// transform's elements [0, W) are stored to grad_in (VRS: added to the Ez terms already there).
// EZ true (VRS, once per chunk): one workgroup per (c, i) runs the chunk's Ez product rows in plane
// order, each lane adding its own elements x x/r_k, y/r_k into grad_in[0], grad_in[1]; the call's
// first plane stores them.  With the two divisions per element the Ez form needs more than the 128
// VGPRs of a 1024-lane workgroup: it is instantiated where rsc_slice_acc_adj is (at most 512 lanes on
// the compile-time plans, Pw = 16384 on the runtime plan) and chosen with it by rss_acc_select.
template <int PN, bool EZ>
__global__ void __launch_bounds__(EZ ? rss_threads_max<PN>() : 1024) rsc_slice_rows_adj(const float2* __restrict__ S, float2* __restrict__ gin,
                                                          FftPlan pw, RscSliceArgs a) {
  extern __shared__ float2 lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int i = blockIdx.x % a.H, c = (blockIdx.x / a.H) % a.C, u = EZ ? 2 : blockIdx.x / (a.H * a.C);
  const size_t prow = (size_t)a.C * a.H * a.Pw;  // one plane of S
  const float2* src = S + u * prow + ((size_t)c * a.H + i) * a.Pw;
  float2* dst = gin + ((size_t)((EZ ? 0 : u) * a.C + c) * a.H + i) * a.W;
  float2* dsty = gin + ((size_t)(a.C + c) * a.H + i) * a.W;  // EZ: the Ey row
  const float xh = lin(-(float)a.H * a.dx / 2.0f, (float)a.H * a.dx / 2.0f, a.H, i);
  const int nk = EZ ? a.nz : 1;
  // element j < W of the inverse transform of chunk plane kk's row
  auto put = [&](int kk, int j, float2 v) {
    if constexpr (!EZ) {
      dst[j] = a.vec ? cadd(dst[j], v) : v;
    } else {
      float2 gx, gy;
      vrs_ez_adj(v, xh, lin(-(float)a.W * a.dx / 2.0f, (float)a.W * a.dx / 2.0f, a.W, j), a.zv[a.zoff + kk], gx, gy);
      const bool st = a.zoff == 0 && kk == 0;
      dst[j] = st ? gx : cadd(dst[j], gx);
      dsty[j] = st ? gy : cadd(dsty[j], gy);
      __builtin_amdgcn_sched_barrier(0);  // one element's divisions at a time
    }
  };
  if constexpr (PN > 0) {
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    for (int kk = 0; kk < nk; ++kk) {
      auto ld = [&](int, int, int j) { return src[kk * prow + j]; };
      auto sv = [&](int, int, int j, float2 v) {
        if (j < a.W) put(kk, j, v);
      };
      fft_pow2_run<true, PN, Geo<PN>::T, FFT_ROWS>(lds, twl, tid, ld, sv);
    }
  } else {
    for (int kk = 0; kk < nk; ++kk) {
      __syncthreads();  // the previous plane's reads of the image are done
      for (int j = tid; j < a.Pw; j += nt) lds[padx(j)] = src[kk * prow + j];
      __syncthreads();
      fft_lds<true>(lds, pw, tid, nt);
      for (int j = tid; j < a.W; j += nt) put(kk, j, lds[padx(j)]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
constexpr int RSS_ZC = 32;  // planes per chunk of the accumulate / line launches

// What a slice call runs with, every part a function of the shape alone: planes per chunk, the tile
// of output planes per accumulate workgroup, the split of the input rows (2048 accumulate workgroups
// per full chunk and tile: eight per CU of two to sixteen waves each), and the workspace parts Uh | P.
// The accumulate launch of a padded width and plane count, decided in this one place: the kernel,
// its block and LDS, and the planes per workgroup the kernel was instantiated for.  The compile-time
// plans tile the Bo planes evenly over ceil(Bo / 3) workgroups (B = 2: one tile of 2, B = 4: two of 2);
// every other width runs the runtime plan, one plane per workgroup.
struct RssAcc {
  void (*k)(const float2*, float2*, FftPlan, RscSliceArgs);
  void (*adj)(const float2*, float2*, FftPlan, RscSliceArgs);  // rsc_slice_acc_adj of the same plan and tile
  void (*ezr)(const float2*, float2*, FftPlan, RscSliceArgs);  // the adjoint's Ez rows on the same plan
  int threads, bt;
  size_t lds;
};
static RssAcc rss_acc_select(int Pw, int Bo) {
  RssAcc r{rsc_slice_acc<0, 1>, rsc_slice_acc_adj<0, 1>, rsc_slice_rows_adj<0, true>, fft_threads(Pw), 1,
           fft_lds_bytes(Pw)};
  on_listed(SizeList<1024, 2048, 4096, 8192>{}, Pw, [&](auto N) {
    static_assert(rss_acc_compiled(N()), "the instantiated accumulate kernels");
    const int nbt = (Bo + RSS_BT_MAX - 1) / RSS_BT_MAX;
    r.bt = (Bo + nbt - 1) / nbt;
    r.k = r.bt == 3 ? rsc_slice_acc<N(), 3> : r.bt == 2 ? rsc_slice_acc<N(), 2> : rsc_slice_acc<N(), 1>;
    r.adj = r.bt == 3   ? rsc_slice_acc_adj<N(), 3>
            : r.bt == 2 ? rsc_slice_acc_adj<N(), 2>
                        : rsc_slice_acc_adj<N(), 1>;
    r.ezr = rsc_slice_rows_adj<N(), true>;
    r.threads = N() / pow2_v(N());
    r.lds = fft_lds_bytes_io(N());
  });
  return r;
}

// The large-LDS opt-in of this unit, once: every instantiation above, with the byte count they had
// on the ASM unit's list (its column pass's k2_lds_bytes(FFT_MAX_N), above every launch here).
static int rsc_slice_lds_attr() {
  static const int rc = [] {
    std::vector<const void*> ks;
    auto family = [&](auto N) {
      constexpr int PN = N();
      ks.insert(ks.end(), {(const void*)rsc_slice_rows<PN>, (const void*)rsc_slice_line<PN>,
                           (const void*)rsc_slice_line_adj<PN>, (const void*)rsc_slice_rows_adj<PN, false>});
      if constexpr (PN == 0 || rss_acc_compiled(PN))
        ks.insert(ks.end(), {(const void*)rsc_slice_acc<PN, 1>, (const void*)rsc_slice_acc_adj<PN, 1>,
                             (const void*)rsc_slice_rows_adj<PN, true>});
      if constexpr (rss_acc_compiled(PN))
        ks.insert(ks.end(), {(const void*)rsc_slice_acc<PN, 2>, (const void*)rsc_slice_acc<PN, 3>,
                             (const void*)rsc_slice_acc_adj<PN, 2>, (const void*)rsc_slice_acc_adj<PN, 3>});
    };
    for_each_size(Pow2Sizes{}, family);
    family(Size<0>{});
    return lds_opt_in(ks, fft_lds_bytes(FFT_MAX_N) + 12 * THZ_MAX_Z);
  }();
  return rc;
}

struct RscSlicePlan {
  RscSliceArgs a;
  RssAcc acc;
  int zc;
  size_t uh, p, gh;  // the forward's Uh | P; the adjoint's S (Uh's shape and size) | Gh
  size_t total() const { return uh + p; }
  size_t total_adj() const { return uh + gh; }
};

static int rsc_slice_plan(const thz_rsc_slice_desc* d, RscSlicePlan* p) {
  if (!d) return fail(THZ_E_ARG, "null descriptor");
  RscSliceArgs& a = p->a;
  int e = rsc_shape(d->B, d->C, d->H, d->W, d->vectorial, d->wavelengths, &a.Ph, &a.Pw);
  if (e) return e;
  if (d->row < 0 || d->row >= a.Ph - d->H)
    return fail(THZ_E_ARG, "RSC slice: row %d outside [0, %d)", d->row, a.Ph - d->H);
  if (d->Z < 1 || d->Z > THZ_MAX_Z) return fail(THZ_E_ARG, "RSC slice: Z=%d outside [1, %d]", d->Z, THZ_MAX_Z);
  if (!d->z) return fail(THZ_E_ARG, "RSC slice: null z");
  a.B = d->B; a.C = d->C; a.H = d->H; a.W = d->W;
  a.vec = d->vectorial != 0;
  a.Bo = a.vec ? 3 : d->B;
  a.row = d->row;
  a.dx = d->dx;
  a.scale = (float)((double)d->dx * (double)d->dy / (double)a.Pw);
  a.nz = a.zoff = 0;
  for (int c = 0; c < d->C; ++c) a.lam[c] = d->wavelengths[c];
  for (int k = 0; k < d->Z; ++k) a.zv[k] = d->z[k];
  p->zc = std::min(d->Z, RSS_ZC);
  p->acc = rss_acc_select(a.Pw, a.Bo);
  a.nbt = (a.Bo + p->acc.bt - 1) / p->acc.bt;
  a.hs = std::max(1, std::min(std::min(d->H, 64), 2048 / (RSS_ZC * d->C)));  // not of B: a plane sums alike in any batch
  const size_t nu = a.vec ? 2 + (size_t)p->zc : (size_t)d->B;
  p->uh = align256(nu * d->C * d->H * a.Pw * sizeof(float2));
  p->p = align256((size_t)p->zc * a.Bo * d->C * a.hs * a.Pw * sizeof(float2));
  p->gh = align256((size_t)p->zc * a.Bo * d->C * a.Pw * sizeof(float2));
  return THZ_OK;
}

// the accumulate launch of the chunk in p.a
static void launch_rss_acc(const RscSlicePlan& p, const float2* Uh, float2* P, const FftPlan& pw, hipStream_t s) {
  const RscSliceArgs& a = p.a;
  hipLaunchKernelGGL(p.acc.k, dim3(a.nz * a.C * a.hs * a.nbt), dim3(p.acc.threads), p.acc.lds, s, Uh, P, pw, a);
}

}  // namespace thz

using namespace thz;

extern "C" int thz_rsc_slice_workspace_size(const thz_rsc_slice_desc* d, size_t* bytes) {
  RscSlicePlan p;
  int e = rsc_slice_plan(d, &p);
  if (e) return e;
  if (!bytes) return fail(THZ_E_ARG, "null bytes");
  *bytes = p.total();
  return THZ_OK;
}

extern "C" int thz_rsc_slice_forward(const thz_rsc_slice_desc* d, const void* in, void* out, void* workspace,
                                     size_t workspace_bytes, thz_stream_t stream) {
  RscSlicePlan p;
  int e = rsc_slice_plan(d, &p);
  if (e) return e;
  if (!in || !out) return fail(THZ_E_ARG, "null data pointer");
  if ((e = check_workspace(workspace, workspace_bytes, p.total()))) return e;
  RscSliceArgs& a = p.a;
  if (a.Pw == a.W) return THZ_OK;  // W = 1: the [..., W:] window is empty
  FftPlan pw;
  if ((e = get_plan(a.Pw, &pw)) || (e = rsc_slice_lds_attr())) return e;
  hipStream_t s = (hipStream_t)stream;
  float2* Uh = (float2*)workspace;
  float2* P = (float2*)((char*)workspace + p.uh);
  const int th = threads_for(a.Pw);
  const size_t lds = fft_lds_bytes_io(a.Pw);
  auto rows = [&](int u0, int nu) {  // Uh planes [u0, u0 + nu)
    KernelTimer kt("rsc_slice_rows", s);
    on_pow2(a.Pw, [&](auto N) {
      hipLaunchKernelGGL(rsc_slice_rows<N()>, dim3(nu * a.C * a.H), dim3(th), lds, s, (const float2*)in, Uh, pw, a, u0);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  };
  if ((e = rows(0, a.vec ? 2 : a.B))) return e;
  for (int k0 = 0; k0 < d->Z; k0 += p.zc) {
    a.zoff = k0;
    a.nz = std::min(p.zc, d->Z - k0);
    if (a.vec && (e = rows(2, a.nz))) return e;  // Ez of the chunk's planes
    {
      KernelTimer kt("rsc_slice_acc", s);
      launch_rss_acc(p, Uh, P, pw, s);
      THZ_LAUNCH_CHECK();
      kt.stop();
    }
    {
      KernelTimer kt("rsc_slice_line", s);
      on_pow2(a.Pw, [&](auto N) {
        hipLaunchKernelGGL(rsc_slice_line<N()>, dim3(a.nz * a.Bo * a.C), dim3(th), lds, s, (const float2*)P,
                           (float2*)out, pw, a);
      });
      THZ_LAUNCH_CHECK();
      kt.stop();
    }
  }
  return THZ_OK;
}

extern "C" int thz_rsc_slice_adjoint_workspace_size(const thz_rsc_slice_desc* d, size_t* bytes) {
  RscSlicePlan p;
  int e = rsc_slice_plan(d, &p);
  if (e) return e;
  if (!bytes) return fail(THZ_E_ARG, "null bytes");
  *bytes = p.total_adj();
  return THZ_OK;
}

extern "C" int thz_rsc_slice_adjoint(const thz_rsc_slice_desc* d, const void* grad_out, void* grad_in,
                                     void* workspace, size_t workspace_bytes, thz_stream_t stream) {
  RscSlicePlan p;
  int e = rsc_slice_plan(d, &p);
  if (e) return e;
  if (!grad_out || !grad_in) return fail(THZ_E_ARG, "null data pointer");
  if ((e = check_workspace(workspace, workspace_bytes, p.total_adj()))) return e;
  RscSliceArgs& a = p.a;
  hipStream_t s = (hipStream_t)stream;
  if (a.Pw == a.W) {  // W = 1: the cotangent is empty and its adjoint zero (the one memset of this entry)
    THZ_HIP_CHECK(hipMemsetAsync(grad_in, 0, (size_t)a.B * a.C * a.H * a.W * sizeof(float2), s));
    return THZ_OK;
  }
  FftPlan pw;
  if ((e = get_plan(a.Pw, &pw)) || (e = rsc_slice_lds_attr())) return e;
  float2* S = (float2*)workspace;
  float2* Gh = (float2*)((char*)workspace + p.uh);
  const int th = threads_for(a.Pw);
  const size_t lds = fft_lds_bytes_io(a.Pw);
  for (int k0 = 0; k0 < d->Z; k0 += p.zc) {
    a.zoff = k0;
    a.nz = std::min(p.zc, d->Z - k0);
    {
      KernelTimer kt("rsc_slice_line_adj", s);
      on_pow2(a.Pw, [&](auto N) {
        hipLaunchKernelGGL(rsc_slice_line_adj<N()>, dim3(a.nz * a.Bo * a.C), dim3(th), lds, s,
                           (const float2*)grad_out, Gh, pw, a);
      });
      THZ_LAUNCH_CHECK();
      kt.stop();
    }
    {
      KernelTimer kt("rsc_slice_acc_adj", s);
      hipLaunchKernelGGL(p.acc.adj, dim3(a.C * a.H * a.nbt), dim3(p.acc.threads), p.acc.lds, s, (const float2*)Gh, S,
                         pw, a);
      THZ_LAUNCH_CHECK();
      kt.stop();
    }
    if (a.vec) {  // the chunk's Ez rows into grad_in[0], grad_in[1]
      KernelTimer kt("rsc_slice_rows_adj", s);
      hipLaunchKernelGGL(p.acc.ezr, dim3(a.C * a.H), dim3(p.acc.threads), p.acc.lds, s, (const float2*)S,
                         (float2*)grad_in, pw, a);
      THZ_LAUNCH_CHECK();
      kt.stop();
    }
  }
  {  // the summed rows, after the last chunk
    KernelTimer kt("rsc_slice_rows_adj", s);
    on_pow2(a.Pw, [&](auto N) {
      hipLaunchKernelGGL((rsc_slice_rows_adj<N(), false>), dim3((a.vec ? 2 : a.B) * a.C * a.H), dim3(th), lds, s,
                         (const float2*)S, (float2*)grad_in, pw, a);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  return THZ_OK;
}
