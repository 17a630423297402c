// Least-squares 2-D phase unwrapping (Ghiglia and Romero): the unweighted solve by a cosine transform, the weighted
// solve by preconditioned conjugate gradients on it, and the residue map (include/thzdoe.h: thz_unwrap_*; unwrap.py;
// DESIGN §42).  Not part of the reference.  The first unit that runs the LDS Stockham engine
// (thz_fft.hpp) on real data: an N-point DCT of TWO real lines is one N-point complex transform.
//
//   packing      A workgroup takes two real lines a, b as z = a + i b.  The engine's first-stage loader reads the
//                operand in Makhoul's order, v[n] = x[2n], v[N - 1 - n] = x[2n + 1], so no permuted copy exists.  With
//                Z = FFT(v_a + i v_b) and m = N - k (Z[N] = Z[0]):
//                    V_a[k] = (Z[k] + conj Z[m]) / 2,   V_b[k] = (Z[k] - conj Z[m]) / 2i,
//                    X[k]   = Re(e^{-i pi k / 2N} V[k])                    (DCT-II, X[k] = sum x[n] cos(pi (2n+1) k / 2N))
//                and back: Z[k] = e^{+i pi k / 2N} ((X_a[k] + X_b[m]) + i (X_b[k] - X_a[m])), X[N] = 0, whose unnormalised
//                inverse transform is N (v_a + i v_b).  The thread of k also owns m, so the combination runs in place in
//                the natural-order LDS line `nat`.  e^{-i pi k / 2N} is entry k of the 4N-point plan's twiddle table
//                (get_plan(4N): made in double on the host, cached per device).
//   rows forward unwrap_rows_fwd: two image rows per workgroup.  The operand is rho formed from the field and the
//                weights in the loader (the neighbouring rows' terms recomputed), or r - alpha Qp in a PCG iteration --
//                the same pass then stores the new r and phi += alpha p.  Output: the rows' DCT-II coefficients.
//   columns      unwrap_cols, in place: the float plane [PH][PW] read as float2 [PH][PW / 2] holds two adjacent columns
//                per element.  DCT-II, division by lambda = -(s_y[k] + s_x[col]) (the (0, 0) term set to 0) and the
//                packing of the DCT-III in one sweep over `nat`, then the inverse transform: the line never leaves LDS.
//   rows inverse unwrap_rows_inv: the inverse packing straight from the two coefficient rows in the loader, stores
//                un-permuted; in PCG it also forms the workgroup's fp64 partial of -(r . z).
//   direction    unwrap_direction: 16 x 64 tiles with a one-pixel halo of p = z + beta p_old and of w in LDS (the halo
//                recomputed), Qp by the weighted five-point stencil, fp64 partial of -(p . Qp).  p is double-buffered:
//                a tile's halo reads its neighbours' old p.
//   scalars      unwrap_scalars (one workgroup per plane) sums the partials in a fixed order and finishes rz, beta,
//                alpha and the freeze; they stay on the device.
//   closing      unwrap_close: the last phi += alpha p, the anchor, congruence and the crop; unwrap_residues: the map.
//
// LDS of a transform workgroup: the engine's image (split exchange + twiddle tables for N >= 1024, the complex image
// of the runtime plan below) followed by nat[N + 1].  4096 points: 53264 B.
// No float atomics, no host sync, no memset: capturable.  Planes ride the grid and every partial count follows the
// shape alone, so a plane's bits do not depend on B.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "thz_common.hpp"
#include "thz_launch.hpp"
#include "thz_stream.hpp"

namespace thz {

constexpr float UW_2PI = 6.28318530717958647692f;
constexpr float UW_INV_2PI = 0.15915494309189533577f;
constexpr int UW_MIN_N = 64, UW_MAX_N = 4096;
constexpr int UW_TY = 16, UW_TX = 64;  // the direction kernel's tile
constexpr int UW_MAX_PARTS = 64;       // partial maxima per plane of the amplitude weights

// What the wrapped differences and the weights are read from.  U or psi (one of them), w or none.
struct UwSrc {
  const float2* U;
  const float* psi;
  const float* w;
  long long wstride;  // elements between the planes of w
  int H, W;
};
struct UwPlane {
  const float2* U;
  const float* psi;
  const float* w;
  int H, W;
};
__device__ __forceinline__ UwPlane uw_plane(const UwSrc& s, int bc) {
  const long long o = (long long)bc * s.H * s.W;
  return UwPlane{s.U ? s.U + o : nullptr, s.psi ? s.psi + o : nullptr, s.w ? s.w + (long long)bc * s.wstride : nullptr,
                 s.H, s.W};
}
// the wrapped phase of pixel b minus that of pixel a (flat indices inside the plane)
__device__ __forceinline__ float uw_diff(const UwPlane& p, int a, int b) {
  if (p.psi) {
    const float d = p.psi[b] - p.psi[a];
    return fmaf(-UW_2PI, rintf(d * UW_INV_2PI), d);
  }
  const float2 c = cmulc(p.U[b], p.U[a]);  // U_b conj U_a
  return atan2f(c.y, c.x);
}
__device__ __forceinline__ float uw_psi(const UwPlane& p, int a) {
  if (p.psi) return p.psi[a];
  const float2 u = p.U[a];
  return atan2f(u.y, u.x);
}
// w of a pixel; 0 outside the plane (the padding of an embedded problem)
__device__ __forceinline__ float uw_w(const UwPlane& p, int i, int j) {
  if (i < 0 || j < 0 || i >= p.H || j >= p.W) return 0.f;
  return p.w ? p.w[i * p.W + j] : 1.f;
}
// weighted wrapped difference of the edge (i, j) - (i, j + 1) / (i, j) - (i + 1, j); 0 where the edge is absent or
// its weight is 0 (the pixels of such an edge are not read)
__device__ __forceinline__ float uw_ex(const UwPlane& p, int i, int j) {
  const float w = fminf(uw_w(p, i, j), uw_w(p, i, j + 1));
  return w > 0.f ? w * uw_diff(p, i * p.W + j, i * p.W + j + 1) : 0.f;
}
__device__ __forceinline__ float uw_ey(const UwPlane& p, int i, int j) {
  const float w = fminf(uw_w(p, i, j), uw_w(p, i + 1, j));
  return w > 0.f ? w * uw_diff(p, i * p.W + j, (i + 1) * p.W + j) : 0.f;
}
__device__ __forceinline__ float uw_rho(const UwPlane& p, int i, int j) {
  return (uw_ex(p, i, j) - uw_ex(p, i, j - 1)) + (uw_ey(p, i, j) - uw_ey(p, i - 1, j));
}

// per-plane PCG scalars
struct UwScal {
  double rz, rz_old, rz0;
  float alpha, beta;
  int frozen, pad;
};

// Makhoul's order: operand n of the transform is sample uw_mk(n) of the line
__device__ __forceinline__ int uw_mk(int n, int N) { return n < (N >> 1) ? 2 * n : 2 * (N - 1 - n) + 1; }

// ---------------------------------------------------------------------------------------------
// The engine behind one interface: ld(idx) -> operand idx, sv(idx, v) <- result idx, natural order both.
// PN > 0: the compile-time split-exchange transform with fused first-stage loads and last-stage stores;
// PN == 0: the runtime plan on the complex image (64 .. 512 points).
// ---------------------------------------------------------------------------------------------
template <int PN>
__host__ __device__ constexpr int uw_image_f2(int n) {
  return PN > 0 ? lds_split_f2(PN) + tw_lds_count(PN) : lds_floats2(n);
}
template <int PN>
struct UwEngine {
  float2* lds;
  FftPlan pl;
  int tid, nt;
  TwLds twl;
  __device__ __forceinline__ UwEngine(float2* l, const FftPlan& p) : lds(l), pl(p), tid(threadIdx.x), nt(blockDim.x) {
    if constexpr (PN > 0) twl = load_tw_lds<PN>(tw_slot<PN>(lds), pl.tw, tid, nt);
  }
  __device__ __forceinline__ float2* nat() const { return lds + uw_image_f2<PN>(pl.n); }
  template <bool INV, class Ld, class Sv>
  __device__ __forceinline__ void run(Ld& ld, Sv& sv) {
    if constexpr (PN > 0) {
      auto l = [&](int, int, int j) { return ld(j); };
      auto s = [&](int, int, int j, float2 v) { sv(j, v); };
      fft_pow2_run<INV, PN, Geo<PN>::T, FFT_ROWS>(lds, twl, tid, l, s);
    } else {
      __syncthreads();  // a previous transform's readers of the image are done
      for (int j = tid; j < pl.n; j += nt) lds[padx(j)] = ld(j);
      __syncthreads();
      fft_lds<INV>(lds, pl, tid, nt);
      for (int j = tid; j < pl.n; j += nt) sv(j, lds[padx(j)]);
    }
  }
};

// DCT-II coefficients k and m = N - k of both lines from nat[k], nat[m] (k = 0 and k = N / 2: m is k's own slot)
struct UwCoef {
  float ak, bk, am, bm;
};
__device__ __forceinline__ UwCoef uw_split(const float2* nat, const float2* __restrict__ q4, int k, int N) {
  const int m = (N - k) & (N - 1);
  const float2 zk = nat[k], zm = nat[m];
  // V_a = (zk + conj zm) / 2, V_b = (zk - conj zm) / 2i; the pair at m is their conjugate
  const float2 va = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
  const float2 vb = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
  const float2 wk = q4[k], wm = q4[k ? N - k : 0];
  UwCoef c;
  c.ak = fmaf(wk.x, va.x, -(wk.y * va.y));
  c.bk = fmaf(wk.x, vb.x, -(wk.y * vb.y));
  c.am = fmaf(wm.x, va.x, wm.y * va.y);  // Re(w_m conj V)
  c.bm = fmaf(wm.x, vb.x, wm.y * vb.y);
  return c;
}
// the DCT-III's packed operand k: conj(w_k) ((a_k + b_m) + i (b_k - a_m)), with X[N] = 0 passed as am = bm = 0
__device__ __forceinline__ float2 uw_pack(float2 wk, float ak, float bk, float am, float bm) {
  return cmulc(make_float2(ak + bm, bk - am), wk);
}

// ---------------------------------------------------------------------------------------------
// Row forward.  mode 0: operand rho (direct solve); 1: rho, and r = rho, phi = 0 (PCG start); 2: r - alpha Qp, the
// new r stored and phi += alpha p.
// ---------------------------------------------------------------------------------------------
struct UwArgs {
  int BC, H, W, PH, PW;
};

template <int PN>
__global__ void __launch_bounds__(256) unwrap_rows_fwd(UwSrc src, UwArgs a, FftPlan pw, const float2* __restrict__ q4,
                                                       float* __restrict__ coef, float* r, const float* __restrict__ qp,
                                                       float* phi, const float* __restrict__ p,
                                                       const UwScal* __restrict__ sc, int mode) {
  extern __shared__ float2 lds[];
  const int half = a.PH >> 1;
  const int bc = blockIdx.x / half, ia = 2 * (blockIdx.x - bc * half);
  const int N = a.PW;
  const size_t row = ((size_t)bc * a.PH + ia) * N;
  UwEngine<PN> eng(lds, pw);
  float2* nat = eng.nat();
  const UwPlane pl = uw_plane(src, bc);
  const float al = mode == 2 ? sc[bc].alpha : 0.f;
  auto ld = [&](int n) {
    const int j = uw_mk(n, N);
    float2 v;
    if (mode == 2) {
      const size_t o = row + j;
      v.x = fmaf(-al, qp[o], r[o]);
      v.y = fmaf(-al, qp[o + N], r[o + N]);
      r[o] = v.x;
      r[o + N] = v.y;
      phi[o] = fmaf(al, p[o], phi[o]);
      phi[o + N] = fmaf(al, p[o + N], phi[o + N]);
    } else {
      v.x = uw_rho(pl, ia, j);
      v.y = uw_rho(pl, ia + 1, j);
      if (mode == 1) {
        const size_t o = row + j;
        r[o] = v.x;
        r[o + N] = v.y;
        phi[o] = 0.f;
        phi[o + N] = 0.f;
      }
    }
    return v;
  };
  auto sv = [&](int k, float2 v) { nat[k] = v; };
  eng.template run<false>(ld, sv);
  __syncthreads();
  for (int k = threadIdx.x; k <= (N >> 1); k += blockDim.x) {
    const UwCoef c = uw_split(nat, q4, k, N);
    coef[row + k] = c.ak;
    coef[row + N + k] = c.bk;
    if (k && k < (N >> 1)) {
      coef[row + N - k] = c.am;
      coef[row + N + N - k] = c.bm;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Column pass, in place: DCT-II down two adjacent columns, / lambda, DCT-III back.
// ---------------------------------------------------------------------------------------------
template <int PN>
__global__ void __launch_bounds__(256) unwrap_cols(UwArgs a, FftPlan ph, const float2* __restrict__ q4,
                                                   const float* __restrict__ sy, const float* __restrict__ sx,
                                                   float2* X, float scale) {
  extern __shared__ float2 lds[];
  const int halfw = a.PW >> 1;
  const int bc = blockIdx.x / halfw, jj = blockIdx.x - bc * halfw;
  const int N = a.PH;
  float2* col = X + (size_t)bc * N * halfw + jj;  // row i at col[i halfw]
  UwEngine<PN> eng(lds, ph);
  float2* nat = eng.nat();
  auto ld0 = [&](int n) { return col[(size_t)uw_mk(n, N) * halfw]; };
  auto sv0 = [&](int k, float2 v) { nat[k] = v; };
  eng.template run<false>(ld0, sv0);
  __syncthreads();
  const float sxa = sx[2 * jj], sxb = sx[2 * jj + 1];
  // X / lambda, lambda = -(s_y + s_x); the sum of non-negatives is 0 at (0, 0) only, where the mean is set to 0
  auto inv = [&](int k, float s) {
    const float d = sy[k] + s;
    return d > 0.f ? -scale / d : 0.f;
  };
  for (int k = threadIdx.x; k <= (N >> 1); k += blockDim.x) {
    UwCoef c = uw_split(nat, q4, k, N);
    const int m = N - k;
    c.ak *= inv(k, sxa);
    c.bk *= inv(k, sxb);
    if (k && k < (N >> 1)) {
      c.am *= inv(m, sxa);
      c.bm *= inv(m, sxb);
      nat[k] = uw_pack(q4[k], c.ak, c.bk, c.am, c.bm);
      nat[m] = uw_pack(q4[m], c.am, c.bm, c.ak, c.bk);
    } else if (k) {  // k = m = N / 2
      nat[k] = uw_pack(q4[k], c.ak, c.bk, c.ak, c.bk);
    } else {
      nat[0] = make_float2(c.ak, c.bk);
    }
  }
  __syncthreads();
  auto ld1 = [&](int k) { return nat[k]; };
  auto sv1 = [&](int n, float2 v) { col[(size_t)uw_mk(n, N) * halfw] = v; };
  eng.template run<true>(ld1, sv1);
}

// ---------------------------------------------------------------------------------------------
// Row inverse, in place on the coefficient rows.  r != null: the workgroup's partial of -(r . z).
// ---------------------------------------------------------------------------------------------
template <int PN>
__global__ void __launch_bounds__(256) unwrap_rows_inv(UwArgs a, FftPlan pw, const float2* __restrict__ q4, float* z,
                                                       const float* __restrict__ r, double* __restrict__ partial) {
  extern __shared__ float2 lds[];
  const int half = a.PH >> 1;
  const int bc = blockIdx.x / half, ia = 2 * (blockIdx.x - bc * half);
  const int N = a.PW;
  float* za = z + ((size_t)bc * a.PH + ia) * N;
  float* zb = za + N;
  UwEngine<PN> eng(lds, pw);
  auto ld = [&](int k) {
    if (k == 0) return make_float2(za[0], zb[0]);
    return uw_pack(q4[k], za[k], zb[k], za[N - k], zb[N - k]);
  };
  Sums<1> acc{};
  const float* ra = r ? r + ((size_t)bc * a.PH + ia) * N : nullptr;
  auto sv = [&](int n, float2 v) {
    const int j = uw_mk(n, N);
    za[j] = v.x;
    zb[j] = v.y;
    if (ra) acc.v[0] -= (double)ra[j] * (double)v.x + (double)ra[j + N] * (double)v.y;
  };
  eng.template run<true>(ld, sv);
  if (ra) store_partials<1>(acc, partial, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// PCG direction: p = z + beta p_old, Qp, the partial of -(p . Qp).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) unwrap_direction(UwSrc src, UwArgs a, const float* __restrict__ z,
                                                        const float* __restrict__ p_old, float* __restrict__ p_new,
                                                        float* __restrict__ qp, const UwScal* __restrict__ sc,
                                                        double* __restrict__ partial, int first) {
  __shared__ float sp[UW_TY + 2][UW_TX + 2];
  __shared__ float sw[UW_TY + 2][UW_TX + 2];
  const int tx = a.PW / UW_TX, ty = a.PH / UW_TY;
  const int bc = blockIdx.x / (tx * ty), t = blockIdx.x - bc * (tx * ty);
  const int i0 = (t / tx) * UW_TY, j0 = (t % tx) * UW_TX;
  const size_t base = (size_t)bc * a.PH * a.PW;
  const UwPlane pl = uw_plane(src, bc);
  const float beta = first ? 0.f : sc[bc].beta;
  for (int e = threadIdx.x; e < (UW_TY + 2) * (UW_TX + 2); e += blockDim.x) {
    const int y = e / (UW_TX + 2), x = e - y * (UW_TX + 2);
    const int i = i0 + y - 1, j = j0 + x - 1;
    float v = 0.f;
    if (i >= 0 && j >= 0 && i < a.PH && j < a.PW) {
      const size_t o = base + (size_t)i * a.PW + j;
      v = first ? z[o] : fmaf(beta, p_old[o], z[o]);
    }
    sp[y][x] = v;
    sw[y][x] = uw_w(pl, i, j);
  }
  __syncthreads();
  Sums<1> acc{};
  for (int e = threadIdx.x; e < UW_TY * UW_TX; e += blockDim.x) {
    const int y = e / UW_TX + 1, x = e % UW_TX + 1;
    const float c = sp[y][x], w = sw[y][x];
    const float q = (fminf(w, sw[y][x + 1]) * (sp[y][x + 1] - c) + fminf(w, sw[y][x - 1]) * (sp[y][x - 1] - c)) +
                    (fminf(w, sw[y + 1][x]) * (sp[y + 1][x] - c) + fminf(w, sw[y - 1][x]) * (sp[y - 1][x] - c));
    const size_t o = base + (size_t)(i0 + y - 1) * a.PW + (j0 + x - 1);
    p_new[o] = c;
    qp[o] = q;
    acc.v[0] -= (double)c * (double)q;
  }
  store_partials<1>(acc, partial, blockIdx.x);
}

// One workgroup per plane.  what 0: rz of iteration k, beta, the freeze, hist; what 1: alpha from p . Qp.
__global__ void __launch_bounds__(256) unwrap_scalars(const double* __restrict__ partial, int parts, UwScal* sc,
                                                      double* __restrict__ hist, int BC, int k, double tol2, int what) {
  const int bc = blockIdx.x;
  const Sums<1> s = gather_partials<1>(partial, parts, (long long)bc * parts);
  if (threadIdx.x) return;
  UwScal v = sc[bc];
  if (what == 0) {
    v.rz = s.v[0];
    if (k == 0) v.rz0 = v.rz;
    // a converged (or broken) step is frozen: without it the iteration breaks down once rz has reached rounding
    v.frozen = !(v.rz > tol2 * v.rz0) || !isfinite(v.rz);
    v.beta = (k == 0 || v.frozen || !(v.rz_old > 0.0)) ? 0.f : (float)(v.rz / v.rz_old);
    v.alpha = 0.f;
    hist[(size_t)k * BC + bc] = v.rz0 > 0.0 ? sqrt(fmax(v.rz, 0.0) / v.rz0) : 0.0;
  } else {
    const double pqp = s.v[0];
    v.alpha = (v.frozen || !(pqp > 0.0) || !isfinite(pqp)) ? 0.f : (float)(v.rz / pqp);
    v.rz_old = v.rz;
  }
  sc[bc] = v;
}

// ---------------------------------------------------------------------------------------------
// Streaming kernels: amplitude / intensity weights, the closing pass, the residue map.  blockIdx.y = plane.
// ---------------------------------------------------------------------------------------------
struct UwMax {
  float v;
  __device__ __forceinline__ void merge(const UwMax& o) { v = fmaxf(v, o.v); }
  __device__ __forceinline__ UwMax shfl_xor(int o) const { return UwMax{__shfl_xor(v, o)}; }
};
__global__ void __launch_bounds__(LANE_THREADS) unwrap_wmax(const float2* __restrict__ U, long long n,
                                                            float* __restrict__ part) {
  const float2* u = U + blockIdx.y * n;
  UwMax m{0.f};
  for (long long e = (long long)blockIdx.x * LANE_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * LANE_THREADS) {
    const float2 c = u[e];
    m.v = fmaxf(m.v, fmaf(c.x, c.x, c.y * c.y));
  }
  m = block_reduce_fixed(m);
  if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = m.v;
}
__global__ void __launch_bounds__(LANE_THREADS) unwrap_wfill(const float2* __restrict__ U, long long n,
                                                             const float* __restrict__ part, int parts, int intensity,
                                                             float* __restrict__ w) {
  float mx = 0.f;
  for (int q = 0; q < parts; ++q) mx = fmaxf(mx, part[blockIdx.y * parts + q]);
  const float2* u = U + blockIdx.y * n;
  float* o = w + blockIdx.y * n;
  const float den = intensity ? mx : sqrtf(mx);
  for (long long e = (long long)blockIdx.x * LANE_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * LANE_THREADS) {
    const float2 c = u[e];
    const float m2 = fmaf(c.x, c.x, c.y * c.y);
    o[e] = den > 0.f ? fminf((intensity ? m2 : sqrtf(m2)) / den, 1.f) : 0.f;
  }
}

struct UwClose {
  int anchor, ar, ac, congruent;
};
__global__ void __launch_bounds__(LANE_THREADS) unwrap_close(UwSrc src, UwArgs a, UwClose c, const float* __restrict__ phi,
                                                             const float* __restrict__ p, const UwScal* __restrict__ sc,
                                                             float* __restrict__ out) {
  const int bc = blockIdx.y;
  const UwPlane pl = uw_plane(src, bc);
  const size_t base = (size_t)bc * a.PH * a.PW;
  const float al = p ? sc[bc].alpha : 0.f;
  auto sol = [&](int i, int j) {
    const size_t o = base + (size_t)i * a.PW + j;
    return p ? fmaf(al, p[o], phi[o]) : phi[o];
  };
  const float shift = c.anchor ? uw_psi(pl, c.ar * a.W + c.ac) - sol(c.ar, c.ac) : 0.f;
  const int n = a.H * a.W;
  float* o = out + (size_t)bc * n;
  for (int e = blockIdx.x * LANE_THREADS + threadIdx.x; e < n; e += gridDim.x * LANE_THREADS) {
    const int i = e / a.W, j = e - i * a.W;
    float v = sol(i, j) + shift;
    if (c.congruent) {
      const float psi = uw_psi(pl, e);
      v = (float)((double)psi + 6.283185307179586476925 * (double)rintf((v - psi) * UW_INV_2PI));
    }
    o[e] = v;
  }
}

__global__ void __launch_bounds__(LANE_THREADS) unwrap_residues(UwSrc src, signed char* __restrict__ out) {
  const UwPlane pl = uw_plane(src, blockIdx.y);
  const int W1 = pl.W - 1, n = (pl.H - 1) * W1;
  signed char* o = out + (size_t)blockIdx.y * n;
  for (int e = blockIdx.x * LANE_THREADS + threadIdx.x; e < n; e += gridDim.x * LANE_THREADS) {
    const int i = e / W1, j = e - i * W1;
    const int a = i * pl.W + j, b = a + 1, c = a + pl.W, d = c + 1;
    const float loop = (uw_diff(pl, a, b) + uw_diff(pl, b, d)) - (uw_diff(pl, c, d) + uw_diff(pl, a, c));
    o[e] = (signed char)rintf(loop * UW_INV_2PI);
  }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
using UwSizes = SizeList<1024, 2048, 4096>;  // compile-time plans; 64 .. 512 run the runtime plan
template <class F>
static void on_uw(int n, F&& f) {
  if (!on_listed(UwSizes{}, n, f)) f(Size<0>{});
}
static bool uw_compiled(int n) { return on_listed(UwSizes{}, n, [](auto) {}); }
static int uw_threads(int n) { return uw_compiled(n) ? n / pow2_v(n) : fft_threads(n); }
static size_t uw_lds(int n) {
  const size_t image = uw_compiled(n) ? lds_split_f2(n) + tw_lds_count(n) : lds_floats2(n);
  return (image + n + 1) * sizeof(float2);
}
static int uw_side(int n) {
  int p = UW_MIN_N;
  while (p < n) p <<= 1;
  return p;
}

// s[k] = 4 sin^2(pi k / 2N), formed in double, stored as fp32, cached per device like get_plan's tables
static int uw_stable(int n, const float** out) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, float*> tabs;
  int dev = 0;
  THZ_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  auto it = tabs.find({dev, n});
  if (it == tabs.end()) {
    std::vector<float> h(n);
    for (int k = 0; k < n; ++k) {
      const double s = std::sin(M_PI * (double)k / (2.0 * (double)n));
      h[k] = (float)(4.0 * s * s);
    }
    float* d = nullptr;
    THZ_HIP_CHECK(hipMalloc(&d, sizeof(float) * n));
    THZ_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    it = tabs.emplace(std::make_pair(dev, n), d).first;
  }
  *out = it->second;
  return THZ_OK;
}

struct UwPlan {
  UwArgs a;
  bool pcg, wplane;
  int tiles, parts, wparts;
  size_t plane, wbytes, partial, wmax, scal;
  size_t total() const { return (pcg ? 6 : 1) * plane + wbytes + partial + wmax + scal; }
};

static int uw_plan(const thz_unwrap_desc* d, UwPlan* p) {
  if (!d) return fail(THZ_E_ARG, "null descriptor");
  if (d->BC < 1 || d->H < 2 || d->W < 2) return fail(THZ_E_ARG, "unwrap: bad shape BC=%d H=%d W=%d", d->BC, d->H, d->W);
  if (d->H > UW_MAX_N || d->W > UW_MAX_N)
    return fail(THZ_E_UNSUPPORTED, "unwrap: plane %dx%d; each side is at most %d", d->H, d->W, UW_MAX_N);
  if (d->BC > 65535) return fail(THZ_E_UNSUPPORTED, "unwrap: BC=%d > 65535 planes", d->BC);
  if (d->input < 0 || d->input > 1) return fail(THZ_E_ARG, "unwrap: input %d is neither field (0) nor phase (1)", d->input);
  if (d->weights < 0 || d->weights > 3) return fail(THZ_E_ARG, "unwrap: bad weights kind %d", d->weights);
  if (d->weights >= 2 && d->input) return fail(THZ_E_ARG, "unwrap: amplitude / intensity weights need a complex field");
  if (d->weights == 1 && d->wstride != 0 && d->wstride != (long long)d->H * d->W)
    return fail(THZ_E_ARG, "unwrap: weight plane stride %lld is neither 0 nor H W", d->wstride);
  if (d->iters < 0 || d->iters > 100000) return fail(THZ_E_ARG, "unwrap: iters=%d", d->iters);
  if (!(d->tol >= 0.0) || !std::isfinite(d->tol)) return fail(THZ_E_ARG, "unwrap: tol must be finite and >= 0");
  if (d->anchor < 0 || d->anchor > 1 ||
      (d->anchor && (d->anchor_row < 0 || d->anchor_row >= d->H || d->anchor_col < 0 || d->anchor_col >= d->W)))
    return fail(THZ_E_ARG, "unwrap: anchor (%d, %d) outside the %dx%d plane", d->anchor_row, d->anchor_col, d->H, d->W);
  UwArgs& a = p->a;
  a.BC = d->BC; a.H = d->H; a.W = d->W; a.PH = uw_side(d->H); a.PW = uw_side(d->W);
  p->pcg = d->iters > 0;
  if (!p->pcg && (d->weights || a.PH != d->H || a.PW != d->W))
    return fail(THZ_E_ARG, "unwrap: the direct solve (iters = 0) takes unweighted planes with power-of-two sides "
                           "from %d; %dx%d%s needs iterations", UW_MIN_N, d->H, d->W, d->weights ? " with weights" : "");
  p->wplane = d->weights >= 2;
  p->tiles = (a.PH / UW_TY) * (a.PW / UW_TX);
  p->parts = std::max(p->tiles, a.PH / 2);
  const long long hw = (long long)d->H * d->W;
  p->wparts = (int)std::min<long long>(UW_MAX_PARTS, (hw + LANE_CHUNK - 1) / LANE_CHUNK);
  if ((long long)d->BC * p->parts > 0x7fffffffLL) return fail(THZ_E_UNSUPPORTED, "unwrap: more than 2^31 - 1 workgroups");
  p->plane = align256((size_t)d->BC * a.PH * a.PW * sizeof(float));
  p->wbytes = p->wplane ? align256((size_t)d->BC * hw * sizeof(float)) : 0;
  p->partial = p->pcg ? align256((size_t)d->BC * p->parts * sizeof(double)) : 0;
  p->wmax = p->wplane ? align256((size_t)d->BC * p->wparts * sizeof(float)) : 0;
  p->scal = p->pcg ? align256((size_t)d->BC * sizeof(UwScal)) : 0;
  return THZ_OK;
}

static int uw_stream_blocks(long long n, int* blocks) {
  return stream_grid((n + LANE_CHUNK - 1) / LANE_CHUNK, blocks);
}

}  // namespace thz

using namespace thz;

extern "C" int thz_unwrap_workspace_size(const thz_unwrap_desc* d, size_t* bytes) {
  UwPlan p;
  int e = uw_plan(d, &p);
  if (e) return e;
  if (!bytes) return fail(THZ_E_ARG, "null bytes");
  *bytes = p.total();
  return THZ_OK;
}

extern "C" int thz_unwrap_phase(const thz_unwrap_desc* d, const void* input, const float* weights, float* out,
                                double* hist, void* workspace, size_t workspace_bytes, thz_stream_t stream) {
  UwPlan P;
  int e = uw_plan(d, &P);
  if (e) return e;
  if ((e = check_arrays("thz_unwrap_phase", {input}, d->input ? 4 : 8))) return e;
  if ((e = check_arrays("thz_unwrap_phase", {out}, 4))) return e;
  if (d->weights == 1 && (e = check_arrays("thz_unwrap_phase", {weights}, 4))) return e;
  if (P.pcg && (e = check_arrays("thz_unwrap_phase", {hist}, 8))) return e;
  if ((e = check_workspace(workspace, workspace_bytes, P.total()))) return e;
  if (misaligned(workspace, 16)) return fail(THZ_E_ARG, "thz_unwrap_phase: workspace not 16-byte aligned");
  const UwArgs& a = P.a;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* zc = (float*)ws;                  // coefficients, then z (PCG) or phi (direct)
  float* phi = (float*)(ws + P.plane);     // the PCG planes: phi, r, p0, p1, Qp
  float* r = (float*)(ws + 2 * P.plane);
  float* pb[2] = {(float*)(ws + 3 * P.plane), (float*)(ws + 4 * P.plane)};
  float* qp = (float*)(ws + 5 * P.plane);
  char* tail = ws + (P.pcg ? 6 : 1) * P.plane;
  float* wpl = (float*)tail;
  double* partial = (double*)(tail + P.wbytes);
  float* wmax = (float*)(tail + P.wbytes + P.partial);
  UwScal* sc = (UwScal*)(tail + P.wbytes + P.partial + P.wmax);

  FftPlan pw, ph, p4w, p4h;
  const float *sx, *sy;
  if ((e = get_plan(a.PW, &pw)) || (e = get_plan(a.PH, &ph)) || (e = get_plan(4 * a.PW, &p4w)) ||
      (e = get_plan(4 * a.PH, &p4h)) || (e = uw_stable(a.PW, &sx)) || (e = uw_stable(a.PH, &sy)))
    return e;

  UwSrc src{d->input ? nullptr : (const float2*)input, d->input ? (const float*)input : nullptr,
            d->weights == 1 ? weights : nullptr, d->weights == 1 ? d->wstride : 0, d->H, d->W};
  const long long hw = (long long)d->H * d->W;
  if (P.wplane) {
    {
      KernelTimer kt("unwrap_wmax", s);
      hipLaunchKernelGGL(unwrap_wmax, dim3(P.wparts, a.BC), dim3(LANE_THREADS), 0, s, src.U, hw, wmax);
      THZ_LAUNCH_CHECK();
      kt.stop();
    }
    int blocks;
    if ((e = uw_stream_blocks(hw, &blocks))) return e;
    KernelTimer kt("unwrap_wfill", s);
    hipLaunchKernelGGL(unwrap_wfill, dim3(blocks, a.BC), dim3(LANE_THREADS), 0, s, src.U, hw, wmax, P.wparts,
                       (int)(d->weights == 3), wpl);
    THZ_LAUNCH_CHECK();
    kt.stop();
    src.w = wpl;
    src.wstride = hw;
  }

  auto rows_fwd = [&](int mode, const float* p) {
    KernelTimer kt("unwrap_rows_fwd", s);
    on_uw(a.PW, [&](auto N) {
      hipLaunchKernelGGL((unwrap_rows_fwd<N()>), dim3(a.BC * (a.PH / 2)), dim3(uw_threads(a.PW)), uw_lds(a.PW), s, src, a,
                         pw, p4w.tw, zc, r, qp, phi, p, sc, mode);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  };
  auto cols = [&]() {
    KernelTimer kt("unwrap_cols", s);
    const float scale = (float)(1.0 / ((double)a.PH * (double)a.PW));
    on_uw(a.PH, [&](auto N) {
      hipLaunchKernelGGL((unwrap_cols<N()>), dim3(a.BC * (a.PW / 2)), dim3(uw_threads(a.PH)), uw_lds(a.PH), s, a, ph,
                         p4h.tw, sy, sx, (float2*)zc, scale);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  };
  auto rows_inv = [&](bool dot) {
    KernelTimer kt("unwrap_rows_inv", s);
    on_uw(a.PW, [&](auto N) {
      hipLaunchKernelGGL((unwrap_rows_inv<N()>), dim3(a.BC * (a.PH / 2)), dim3(uw_threads(a.PW)), uw_lds(a.PW), s, a, pw,
                         p4w.tw, zc, dot ? (const float*)r : nullptr, partial);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  };
  auto scalars = [&](int parts, int k, int what) {
    KernelTimer kt("unwrap_scalars", s);
    hipLaunchKernelGGL(unwrap_scalars, dim3(a.BC), dim3(256), 0, s, partial, parts, sc, hist, a.BC, k, d->tol * d->tol,
                       what);
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  };

  const float* plast = nullptr;
  if (!P.pcg) {
    if ((e = rows_fwd(0, nullptr)) || (e = cols()) || (e = rows_inv(false))) return e;
  } else {
    for (int k = 0; k < d->iters; ++k) {
      float* pn = pb[k & 1];
      if ((e = rows_fwd(k ? 2 : 1, plast)) || (e = cols()) || (e = rows_inv(true)) || (e = scalars(a.PH / 2, k, 0)))
        return e;
      {
        KernelTimer kt("unwrap_direction", s);
        hipLaunchKernelGGL(unwrap_direction, dim3(a.BC * P.tiles), dim3(256), 0, s, src, a, zc, plast, pn, qp, sc, partial,
                           (int)(k == 0));
        THZ_LAUNCH_CHECK();
        kt.stop();
      }
      if ((e = scalars(P.tiles, k, 1))) return e;
      plast = pn;
    }
  }
  int blocks;
  if ((e = uw_stream_blocks(hw, &blocks))) return e;
  KernelTimer kt("unwrap_close", s);
  const UwClose c{d->anchor, d->anchor_row, d->anchor_col, d->congruent};
  hipLaunchKernelGGL(unwrap_close, dim3(blocks, a.BC), dim3(LANE_THREADS), 0, s, src, a, c, P.pcg ? phi : zc, plast, sc,
                     out);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_unwrap_residues(int BC, int H, int W, int input_kind, const void* input, signed char* out,
                                   thz_stream_t stream) {
  if (BC < 1 || H < 2 || W < 2) return fail(THZ_E_ARG, "unwrap residues: bad shape BC=%d H=%d W=%d", BC, H, W);
  if (BC > 65535 || (long long)H * W > 0x7fffffffLL)
    return fail(THZ_E_UNSUPPORTED, "unwrap residues: BC=%d > 65535 planes or H W above 2^31 - 1", BC);
  if (input_kind < 0 || input_kind > 1) return fail(THZ_E_ARG, "unwrap residues: input %d", input_kind);
  int e;
  if ((e = check_arrays("thz_unwrap_residues", {input}, input_kind ? 4 : 8))) return e;
  if ((e = check_arrays("thz_unwrap_residues", {out}, 1))) return e;
  const UwSrc src{input_kind ? nullptr : (const float2*)input, input_kind ? (const float*)input : nullptr, nullptr, 0, H,
                  W};
  int blocks;
  if ((e = uw_stream_blocks((long long)(H - 1) * (W - 1), &blocks))) return e;
  KernelTimer kt("unwrap_residues", (hipStream_t)stream);
  hipLaunchKernelGGL(unwrap_residues, dim3(blocks, BC), dim3(LANE_THREADS), 0, (hipStream_t)stream, src, out);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
