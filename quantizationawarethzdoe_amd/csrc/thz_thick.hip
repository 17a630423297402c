// Thick-element DOE model for gfx950: split-step (multi-slice) propagation through the relief.  The
// reference has no counterpart; a slab's screen is DOELayer.modulate's (Components/QuantizedDOE.py:
// 47-126) on the slab's share of the height, a step is ASM_prop.forward over dz (Props/ASM_Prop.py:
// 314-378).  This unit shares with the ASM unit the exported transfer function (thz_asm_transfer_function)
// and the host toolkit (thz_launch.hpp), no kernel.
#include <algorithm>
#include <cmath>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_launch.hpp"

namespace thz {

// ---------------------------------------------------------------------------------------------
// With dz = T / S, z_s = s dz, d_s = clamp(h_full - z_s, 0, dz) (d_0 on the base plate) and
// t_{c,s} = exp(-k_c/2 d_s tand sqrt(eps)) exp(sign i k_c d_s (sqrt(eps) - 1)):
//   U_{s+1} = crop(IFFT2(FFT2(pad(U_s t_s)) H_dz)),  s = 0 .. S-1
// The window sits at the origin of the padded plane (a circular convolution does not see where the
// window lies, and loads and crops then need no offset).  Rows outside the window are zero after
// every crop, so the intermediate X keeps the H window rows only, as row spectra [BC][H][Pw] in
// column blocks of CB columns (blk: a row pass touches 128-B segments, a column workgroup one
// 8-B element per segment, the CB workgroups of a block back to back on one XCD).
//   thick_rows<first>  : U_0 row x t_0 -> zero-padded FFT_Pw -> X
//   thick_cols         : X column (H values, zero-padded) -> FFT_Ph -> x H_dz column -> IFFT_Ph ->
//                        x 1/(Ph Pw) -> the H window values back in place
//   thick_rows<middle> : X row -> IFFT_Pw -> the W window values x t_s, zero elsewhere -> FFT_Pw -> X
//                        (the inverse hands its results to the forward in registers on the
//                        compile-time plans: the slab's spatial field never goes to memory)
//   thick_rows<last>   : X row -> IFFT_Pw -> the W window values -> out
// S + 1 row launches and S column launches per call; H_dz is one table [C][Ph][Pw] on the centred
// grid for every slab, read with the shift folded into the index.
//
// Backward.  A step is A = crop F^-1 diag(H_dz) F pad, so A^H = crop F^-1 diag(conj H_dz) F pad (the
// 1/N cancel): the same passes with the table read conjugated.  d_s has a non-zero derivative in h
// only in the one slab the pixel's height ends in (its active slab, thick_active), where t_s' =
// kappa_c t_s, kappa_c = -(k_c/2) tand sqrt(eps) + sign i k_c (sqrt(eps) - 1).  With V_s = U_s t_s:
//   gV_s = A^H gU_{s+1},  gU_s = conj(t_s) gV_s,  g_h(p) = sum_bc Re(conj(kappa_c V_s(p)) gV_s(p)), s = s(p)
// so the saving forward keeps one field-sized stash, V_s(p) where s is the active slab of p, and the
// backward writes one partial per (bc, pixel) where the pixel has an active slab:
//   thick_grad_rows<first>  : grad_out row -> zero-padded FFT_Pw -> X
//   thick_cols<conj>        : as above with conj H_dz
//   thick_grad_rows<middle> : X row -> IFFT_Pw -> gV_s on the window -> partial where s is active ->
//                             x conj(t_s), zero elsewhere -> FFT_Pw -> X  (s = S-1 .. 1)
//   thick_grad_rows<last>   : X row -> IFFT_Pw -> gV_0 -> partial, grad_field = conj(t_0) gV_0
//   thick_grad_reduce       : partials -> grad_height [hs][ws]: fp64 sums over bc and the nearest-
//                             upsample footprint in a fixed order; pixels without an active slab are
//                             told from h itself and give 0, so the partials need no memset
// ---------------------------------------------------------------------------------------------
struct ThickArgs {
  int BC, C, H, W, Ph, Pw, hs, ws;
  int xr;      // rows of a column block of X: H, or H + 1 where H rows are a multiple of 4096 B
  int base;    // 1: this slab carries the base plate (s = 0)
  float zs, dz;  // the slab's lower face and thickness
  float zn;      // the next slab's lower face; +inf on the last slab
  float eps, tand, sign, scale;
  float lam[THZ_MAX_WAVELENGTHS];
};

constexpr int THICK_FIRST = 0, THICK_MIDDLE = 1, THICK_LAST = 2;

// h - z_s in fp32: the one expression the screen and the active-slab rule are built on.
__device__ __forceinline__ float thick_rise(float h, float zs) { return h - zs; }

// The active slab of a pixel, the one whose d_s = clamp(h - z_s, 0, dz) moves with h: 0 < h - z_s < dz
// on the fp32 values thick_screen clamps.  Where the fp32 faces let two neighbouring slabs pass that
// test (h within an ulp of a face), the upper one is the active slab, so a pixel has at most one.
__device__ __forceinline__ bool thick_in(float h, float zs, float dz) {
  const float x = thick_rise(h, zs);
  return x > 0.f && x < dz;
}
__device__ __forceinline__ bool thick_active(const ThickArgs& a, float h) {
  return thick_in(h, a.zs, a.dz) && !thick_in(h, a.zn, a.dz);
}

// t_{c,s} at a pixel of height h.  doe_transmission adds the base plate to its argument, so a slab
// above the first hands it d_s - b, as a caller of thz_doe_modulate_forward would.
__device__ __forceinline__ float2 thick_screen(const ThickArgs& a, float h, float lam) {
  const float d = fminf(fmaxf(thick_rise(h, a.zs), 0.f), a.dz);
  float2 t = doe_transmission(a.base ? d : d - DOE_BASE_PLANE, lam, a.eps, a.tand, nullptr);
  t.y = -a.sign * t.y;  // doe_transmission's phase is the sign = -1 one
  return t;
}

// SAVE (first and middle): `out` is the stash, and V_s = U_s t_s goes to it where s is the pixel's active
// slab; the values handed on are those of the plain pass.
template <int PN, int MODE, bool SAVE = false>
__global__ void __launch_bounds__(1024) thick_rows(const float2* __restrict__ in, const float* __restrict__ hmap,
                                                  float2* X, float2* __restrict__ out, FftPlan pw, ThickArgs a) {
  static_assert(!SAVE || MODE != THICK_LAST, "the last pass has no screen");
  extern __shared__ float2 lds[];
  int tid = threadIdx.x;
  const int nt = blockDim.x;
  const int bc = blockIdx.x / a.H, i = blockIdx.x - bc * a.H;
  const float lam = a.lam[bc % a.C];
  const float* hrow = hmap + (size_t)doe_nearest_src(i, a.hs, a.H) * a.ws;
  const float2* src = in + ((size_t)bc * a.H + i) * a.W;
  float2* dst = out + ((size_t)bc * a.H + i) * a.W;
  float2* xrow = X + (size_t)bc * a.Pw * a.xr + blk(0, i, a.xr);
  auto xoff = [&](int j) { return (size_t)(j / CB) * a.xr * CB + (j % CB); };
  auto screen = [&](int j) { return thick_screen(a, hrow[doe_nearest_src(j, a.ws, a.W)], lam); };
  auto keep = [&](int j, float2 v) {
    if constexpr (SAVE)
      if (thick_active(a, hrow[doe_nearest_src(j, a.ws, a.W)])) dst[j] = v;
    return v;
  };
  auto first = [&](int j) { return j < a.W ? keep(j, cmul(src[j], screen(j))) : make_float2(0.f, 0.f); };
  auto slab = [&](int j, float2 v) { return j < a.W ? keep(j, cmul(v, screen(j))) : make_float2(0.f, 0.f); };
  if constexpr (PN > 0) {
    constexpr int TT = Geo<PN>::T;
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    auto ldx = [&](int, int, int j) { return xrow[xoff(j)]; };
    auto svx = [&](int, int, int j, float2 v) { xrow[xoff(j)] = v; };
    if constexpr (MODE == THICK_FIRST) {
      auto ld = [&](int, int, int j) { return first(j); };
      fft_pow2_run<false, PN, TT, FFT_ROWS>(lds, twl, tid, ld, svx);
    } else if constexpr (MODE == THICK_LAST) {
      auto sv = [&](int, int, int j, float2 v) {
        if (j < a.W) dst[j] = v;
      };
      fft_pow2_run<true, PN, TT, FFT_ROWS>(lds, twl, tid, ldx, sv);
    } else {
      // the inverse (remainder radix last) hands element (m, r) to the forward (remainder radix
      // first) in registers: both index it i + r N / R
      using S = Pow2Sched<PN>;
      constexpr int RL = S::radix(S::NST - 1, 0);
      constexpr int MBL = PN / RL / TT;
      float2 sp[MBL][RL];
      auto sv0 = [&](int mm, int r, int, float2 v) { sp[mm][r] = v; };
      fft_pow2_run<true, PN, TT, 0>(lds, twl, tid, ldx, sv0);
      asm volatile("" : "+v"(tid));
      auto ld1 = [&](int mm, int r, int j) { return slab(j, sp[mm][r]); };
      fft_pow2_run<false, PN, TT, 1>(lds, twl, tid, ld1, svx);
    }
  } else {
    const int n = a.Pw;
    for (int j = tid; j < n; j += nt) lds[padx(j)] = MODE == THICK_FIRST ? first(j) : xrow[xoff(j)];
    __syncthreads();
    if constexpr (MODE != THICK_FIRST) {
      fft_lds<true>(lds, pw, tid, nt);
      if constexpr (MODE == THICK_LAST) {
        for (int j = tid; j < a.W; j += nt) dst[j] = lds[padx(j)];
        return;
      }
      for (int j = tid; j < n; j += nt) lds[padx(j)] = slab(j, lds[padx(j)]);
      __syncthreads();
    }
    fft_lds<false>(lds, pw, tid, nt);
    for (int j = tid; j < n; j += nt) xrow[xoff(j)] = lds[padx(j)];
  }
}

// The backward's row passes (the launch order and the formulas: the head of this file).  part and
// gfield may be null: no height gradient (the stash is then not read), no field gradient.
template <int PN, int MODE>
__global__ void __launch_bounds__(1024) thick_grad_rows(const float2* __restrict__ gout, const float* __restrict__ hmap,
                                                       float2* X, const float2* __restrict__ stash,
                                                       float2* __restrict__ gfield, float* __restrict__ part, FftPlan pw,
                                                       ThickArgs a) {
  extern __shared__ float2 lds[];
  int tid = threadIdx.x;
  const int nt = blockDim.x;
  const int bc = blockIdx.x / a.H, i = blockIdx.x - bc * a.H;
  const float lam = a.lam[bc % a.C];
  const size_t row = ((size_t)bc * a.H + i) * a.W;
  const float* hrow = hmap + (size_t)doe_nearest_src(i, a.hs, a.H) * a.ws;
  float2* xrow = X + (size_t)bc * a.Pw * a.xr + blk(0, i, a.xr);
  auto xoff = [&](int j) { return (size_t)(j / CB) * a.xr * CB + (j % CB); };
  // kappa_c in doe_transmission's operation order (its gamma), the phase term with the convention's sign
  float2 kappa;
  doe_transmission(0.f, lam, a.eps, a.tand, &kappa);
  kappa.y = -a.sign * kappa.y;
  // gV_s at window column j: the height partial where s is the active slab, then gU_s = conj(t_s) gV_s
  auto adj = [&](int j, float2 g) {
    const float h = hrow[doe_nearest_src(j, a.ws, a.W)];
    if (part && thick_active(a, h)) {
      const float2 kv = cmul(kappa, stash[row + j]);
      part[row + j] = __builtin_fmaf(kv.x, g.x, kv.y * g.y);  // Re(conj(kappa V) gV)
    }
    return cmulc(g, thick_screen(a, h, lam));
  };
  auto slab = [&](int j, float2 g) { return j < a.W ? adj(j, g) : make_float2(0.f, 0.f); };
  auto first = [&](int j) { return j < a.W ? gout[row + j] : make_float2(0.f, 0.f); };
  auto last = [&](int j, float2 g) {
    if (j >= a.W) return;
    g = adj(j, g);
    if (gfield) gfield[row + j] = g;
  };
  if constexpr (PN > 0) {
    constexpr int TT = Geo<PN>::T;
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    auto ldx = [&](int, int, int j) { return xrow[xoff(j)]; };
    auto svx = [&](int, int, int j, float2 v) { xrow[xoff(j)] = v; };
    if constexpr (MODE == THICK_FIRST) {
      auto ld = [&](int, int, int j) { return first(j); };
      fft_pow2_run<false, PN, TT, FFT_ROWS>(lds, twl, tid, ld, svx);
    } else if constexpr (MODE == THICK_LAST) {
      auto sv = [&](int, int, int j, float2 v) { last(j, v); };
      fft_pow2_run<true, PN, TT, FFT_ROWS>(lds, twl, tid, ldx, sv);
    } else {
      // the register hand-over of thick_rows<middle>
      using S = Pow2Sched<PN>;
      constexpr int RL = S::radix(S::NST - 1, 0);
      constexpr int MBL = PN / RL / TT;
      float2 sp[MBL][RL];
      auto sv0 = [&](int mm, int r, int, float2 v) { sp[mm][r] = v; };
      fft_pow2_run<true, PN, TT, 0>(lds, twl, tid, ldx, sv0);
      asm volatile("" : "+v"(tid));
      auto ld1 = [&](int mm, int r, int j) { return slab(j, sp[mm][r]); };
      fft_pow2_run<false, PN, TT, 1>(lds, twl, tid, ld1, svx);
    }
  } else {
    const int n = a.Pw;
    for (int j = tid; j < n; j += nt) lds[padx(j)] = MODE == THICK_FIRST ? first(j) : xrow[xoff(j)];
    __syncthreads();
    if constexpr (MODE != THICK_FIRST) {
      fft_lds<true>(lds, pw, tid, nt);
      if constexpr (MODE == THICK_LAST) {
        for (int j = tid; j < a.W; j += nt) last(j, lds[padx(j)]);
        return;
      }
      for (int j = tid; j < n; j += nt) lds[padx(j)] = slab(j, lds[padx(j)]);
      __syncthreads();
    }
    fft_lds<false>(lds, pw, tid, nt);
    for (int j = tid; j < n; j += nt) xrow[xoff(j)] = lds[padx(j)];
  }
}

// grad_height[r][c] = the sum of the partials over bc and over the window pixels whose nearest source
// is (r, c), in fp64 and in a fixed order: the G lanes of a map pixel each sum every G-th term, then a
// tree over the lanes.  A height without an active slab gives 0 and no partial is read: none was written.
struct ThickReduceArgs {
  int BC, H, W, hs, ws, S, G;  // G: lanes per map pixel, a power of two <= THICK_REDUCE_THREADS
  float dzf;
  double dz;
};
constexpr int THICK_REDUCE_THREADS = 256;

// first window index in [0, n) whose nearest source is >= r (doe_nearest_src is monotone), or n
__device__ __forceinline__ int thick_footprint(int r, int in, int n) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (doe_nearest_src(mid, in, n) >= r) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__global__ void __launch_bounds__(THICK_REDUCE_THREADS) thick_grad_reduce(const float* __restrict__ part,
                                                                         const float* __restrict__ hmap,
                                                                         float* __restrict__ gh, ThickReduceArgs a) {
  __shared__ double sums[THICK_REDUCE_THREADS];
  const int tid = threadIdx.x, lane = tid % a.G;
  const long long pix = (long long)blockIdx.x * (THICK_REDUCE_THREADS / a.G) + tid / a.G;
  const bool live = pix < (long long)a.hs * a.ws;
  double acc = 0.0;
  if (live) {
    const int r = (int)(pix / a.ws), c = (int)(pix - (long long)r * a.ws);
    const float h = hmap[pix];
    bool active = false;
    for (int s = 0; s < a.S; ++s) active = active || thick_in(h, (float)((double)s * a.dz), a.dzf);
    if (active) {
      const int i0 = thick_footprint(r, a.hs, a.H), i1 = thick_footprint(r + 1, a.hs, a.H);
      const int j0 = thick_footprint(c, a.ws, a.W), j1 = thick_footprint(c + 1, a.ws, a.W);
      const int nj = j1 - j0;
      const long long per = (long long)(i1 - i0) * nj, n = per * a.BC;
      for (long long e = lane; e < n; e += a.G) {
        const int bc = (int)(e / per);
        const long long q = e - (long long)bc * per;
        const int di = (int)(q / nj), dj = (int)(q - (long long)di * nj);
        acc += (double)part[((size_t)bc * a.H + i0 + di) * a.W + j0 + dj];
      }
    }
  }
  sums[tid] = acc;
  __syncthreads();
  for (int w = a.G >> 1; w > 0; w >>= 1) {
    if (lane < w) sums[tid] += sums[tid + w];
    __syncthreads();
  }
  if (live && lane == 0) gh[pix] = (float)sums[tid];
}

// One workgroup per (bc, spectral column j), in place on the column's H window values.  CONJ: the
// table read conjugated, the column pass of the adjoint step.
template <int PN, bool CONJ = false>
__global__ void __launch_bounds__(1024) thick_cols(float2* X, const float2* __restrict__ tab, FftPlan ph, ThickArgs a) {
  extern __shared__ float2 lds[];
  int tid = threadIdx.x;
  const int nt = blockDim.x;
  const int id = xcd_chunk(blockIdx.x, gridDim.x);
  const int bc = id / a.Pw, j = id - bc * a.Pw;
  float2* col = X + (size_t)bc * a.Pw * a.xr + blk(j, 0, a.xr);  // row i at col[i CB]
  // H on the centred grid: natural frequency index m lives at (m + P / 2) mod P on either axis
  const float2* tcol = tab + (size_t)(bc % a.C) * a.Ph * a.Pw + ((j + a.Pw / 2) & (a.Pw - 1));
  auto load = [&](int i) { return i < a.H ? col[(size_t)i * CB] : make_float2(0.f, 0.f); };
  auto tf = [&](int m) { return tcol[(size_t)((m + a.Ph / 2) & (a.Ph - 1)) * a.Pw]; };
  auto times = [](float2 v, float2 h) { return CONJ ? cmulc(v, h) : cmul(v, h); };
  auto store = [&](int i, float2 v) {
    if (i < a.H) col[(size_t)i * CB] = cscale(v, a.scale);
  };
  if constexpr (PN > 0) {
    using S = Pow2Sched<PN>;
    constexpr int TT = Geo<PN>::T;
    constexpr int RL = S::radix(S::NST - 1, 0);
    constexpr int MBL = PN / RL / TT;
    float2 sp[MBL][RL];
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), ph.tw, tid, nt);
    auto ld0 = [&](int, int, int i) { return load(i); };
    auto sv0 = [&](int mm, int r, int, float2 v) { sp[mm][r] = v; };
    fft_pow2_run<false, PN, TT, 0>(lds, twl, tid, ld0, sv0);
    asm volatile("" : "+v"(tid));
    auto ld1 = [&](int mm, int r, int m) { return times(sp[mm][r], tf(m)); };
    auto sv1 = [&](int, int, int i, float2 v) { store(i, v); };
    fft_pow2_run<true, PN, TT, 1>(lds, twl, tid, ld1, sv1);
  } else {
    const int n = a.Ph;
    for (int i = tid; i < n; i += nt) lds[padx(i)] = load(i);
    __syncthreads();
    fft_lds<false>(lds, ph, tid, nt);
    for (int m = tid; m < n; m += nt) lds[padx(m)] = times(lds[padx(m)], tf(m));
    __syncthreads();
    fft_lds<true>(lds, ph, tid, nt);
    for (int i = tid; i < a.H; i += nt) store(i, lds[padx(i)]);
  }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
constexpr int THICK_MIN_N = 64, THICK_MAX_N = 8192, THICK_MAX_SLICES = 256;
using ThickSizes = SizeList<1024, 2048, 4096, 8192>;  // the compile-time plans; 64 .. 512 run the runtime plan

template <class F>
static void on_thick(int n, F&& f) {
  if (!on_listed(ThickSizes{}, n, f)) f(Size<0>{});
}
static bool thick_compiled(int n) { return on_listed(ThickSizes{}, n, [](auto) {}); }
static int thick_threads(int n) { return thick_compiled(n) ? n / pow2_v(n) : fft_threads(n); }
static size_t thick_lds(int n) { return thick_compiled(n) ? fft_lds_bytes_io(n) : fft_lds_bytes(n); }
static bool thick_length(int n) { return n >= THICK_MIN_N && n <= THICK_MAX_N && (n & (n - 1)) == 0; }

struct ThickPlan {
  ThickArgs a;
  int S;
  double dz;        // T / S of the fp32 thickness, in double: z_s = (float)(s dz)
  size_t x, tab;    // the workspace parts X | H_dz
  size_t total() const { return x + tab; }
};

static int thick_plan(const thz_thick_desc* d, ThickPlan* p) {
  if (!d) return fail(THZ_E_ARG, "null descriptor");
  if (d->B < 1 || d->C < 1 || d->H < 1 || d->W < 1 || d->pad_h < 0 || d->pad_w < 0 || d->hs < 1 || d->ws < 1)
    return fail(THZ_E_ARG, "thick DOE: bad shape B=%d C=%d H=%d W=%d pad=(%d,%d) map=%dx%d", d->B, d->C, d->H, d->W,
                d->pad_h, d->pad_w, d->hs, d->ws);
  if (d->slices < 1) return fail(THZ_E_ARG, "thick DOE: slices=%d < 1", d->slices);
  if (!(d->thickness > 0.f) || !std::isfinite(d->thickness))
    return fail(THZ_E_ARG, "thick DOE: the thickness must be a positive length");
  if (!(std::fabs(d->phase_sign) == 1.f)) return fail(THZ_E_ARG, "thick DOE: phase_sign must be +1 or -1");
  if (d->bandlimit < 0 || d->bandlimit > 2) return fail(THZ_E_ARG, "thick DOE: bad bandlimit %d", d->bandlimit);
  if (!d->wavelengths) return fail(THZ_E_ARG, "thick DOE: null wavelengths");
  if (!(d->dx > 0.f) || !(d->dy > 0.f)) return fail(THZ_E_ARG, "thick DOE: spacing must be > 0");
  if (!(d->epsilon > 0.f) || !(d->tand == d->tand)) return fail(THZ_E_ARG, "thick DOE: bad epsilon / tand");
  if (d->C > THZ_MAX_WAVELENGTHS)
    return fail(THZ_E_UNSUPPORTED, "thick DOE: C=%d > %d wavelengths", d->C, THZ_MAX_WAVELENGTHS);
  for (int c = 0; c < d->C; ++c)
    if (!(d->wavelengths[c] > 0.f)) return fail(THZ_E_ARG, "thick DOE: wavelength[%d] must be > 0", c);
  const long long Ph = (long long)d->H + 2LL * d->pad_h, Pw = (long long)d->W + 2LL * d->pad_w;
  if (Ph > THICK_MAX_N || Pw > THICK_MAX_N || !thick_length((int)Ph) || !thick_length((int)Pw))
    return fail(THZ_E_UNSUPPORTED, "thick DOE: padded plane %lldx%lld; each side must be a power of two in [%d, %d]", Ph,
                Pw, THICK_MIN_N, THICK_MAX_N);
  if (d->slices > THICK_MAX_SLICES)
    return fail(THZ_E_UNSUPPORTED, "thick DOE: slices=%d > %d", d->slices, THICK_MAX_SLICES);
  const long long BC = (long long)d->B * d->C;
  if (BC * std::max(Pw, (long long)d->H) > 0x7fffffffLL)
    return fail(THZ_E_UNSUPPORTED, "thick DOE: more than 2^31 - 1 workgroups");
  ThickArgs& a = p->a;
  a.BC = (int)BC; a.C = d->C; a.H = d->H; a.W = d->W; a.Ph = (int)Ph; a.Pw = (int)Pw; a.hs = d->hs; a.ws = d->ws;
  a.xr = d->H + (((size_t)d->H * CB * sizeof(float2)) % 4096 == 0 ? 1 : 0);
  a.base = 1;
  p->S = d->slices;
  p->dz = (double)d->thickness / (double)d->slices;
  a.zs = 0.f;
  a.zn = INFINITY;
  a.dz = (float)p->dz;
  a.eps = d->epsilon; a.tand = d->tand; a.sign = d->phase_sign;
  a.scale = (float)(1.0 / ((double)Ph * (double)Pw));
  for (int c = 0; c < d->C; ++c) a.lam[c] = d->wavelengths[c];
  p->x = align256((size_t)BC * Pw * a.xr * sizeof(float2));
  p->tab = align256((size_t)d->C * Ph * Pw * sizeof(float2));
  return THZ_OK;
}

}  // namespace thz

using namespace thz;

extern "C" int thz_thick_workspace_size(const thz_thick_desc* d, size_t* bytes) {
  ThickPlan p;
  int e = thick_plan(d, &p);
  if (e) return e;
  if (!bytes) return fail(THZ_E_ARG, "null bytes");
  *bytes = p.total();
  return THZ_OK;
}

namespace thz {

// the slab the next row pass applies: its faces, and whether it carries the base plate
static void thick_slab(ThickPlan& p, int sl) {
  ThickArgs& a = p.a;
  a.base = sl == 0;
  a.zs = (float)((double)sl * p.dz);
  a.zn = sl + 1 < p.S ? (float)((double)(sl + 1) * p.dz) : INFINITY;
}

// H of one step into tab, the table ASM_prop.create_kernel exports for z = dz
static int thick_table(const thz_thick_desc* d, const ThickArgs& a, float2* tab, thz_stream_t stream) {
  const float zstep = a.dz;
  thz_asm_desc ad{};
  ad.B = d->B; ad.C = d->C; ad.H = d->H; ad.W = d->W; ad.pad_h = d->pad_h; ad.pad_w = d->pad_w;
  ad.unpad = 1; ad.bandlimit = d->bandlimit; ad.Z = 1;
  ad.dx = d->dx; ad.dy = d->dy; ad.wavelengths = d->wavelengths; ad.z = &zstep;
  return thz_asm_transfer_function(&ad, tab, stream);
}

template <bool CONJ>
static int thick_cols_launch(const ThickArgs& a, float2* X, const float2* tab, const FftPlan& ph, hipStream_t s) {
  KernelTimer kt(CONJ ? "thick_grad_cols" : "thick_cols", s);
  on_thick(a.Ph, [&](auto N) {
    hipLaunchKernelGGL((thick_cols<N(), CONJ>), dim3(a.BC * a.Pw), dim3(thick_threads(a.Ph)), thick_lds(a.Ph), s, X, tab,
                       ph, a);
  });
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

// stash == null: thz_thick_forward; else the first and middle row passes are the saving ones
static int thick_forward(const thz_thick_desc* d, ThickPlan& p, const void* field, const float* height, void* out,
                         void* stash, void* workspace, thz_stream_t stream) {
  int e;
  ThickArgs& a = p.a;
  hipStream_t s = (hipStream_t)stream;
  float2* X = (float2*)workspace;
  float2* tab = (float2*)((char*)workspace + p.x);
  if ((e = thick_table(d, a, tab, stream))) return e;
  FftPlan pw, ph;
  if ((e = get_plan(a.Pw, &pw)) || (e = get_plan(a.Ph, &ph))) return e;
  auto rows = [&](int mode) {
    const bool save = stash && mode != THICK_LAST;
    KernelTimer kt(save ? "thick_rows_saved" : "thick_rows", s);
    on_thick(a.Pw, [&](auto N) {
      auto k = mode == THICK_LAST    ? thick_rows<N(), THICK_LAST>
               : mode == THICK_FIRST ? (save ? thick_rows<N(), THICK_FIRST, true> : thick_rows<N(), THICK_FIRST>)
                                     : (save ? thick_rows<N(), THICK_MIDDLE, true> : thick_rows<N(), THICK_MIDDLE>);
      hipLaunchKernelGGL(k, dim3(a.BC * a.H), dim3(thick_threads(a.Pw)), thick_lds(a.Pw), s, (const float2*)field, height,
                         X, (float2*)(save ? stash : out), pw, a);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  };
  thick_slab(p, 0);
  if ((e = rows(THICK_FIRST))) return e;
  for (int sl = 0; sl < p.S; ++sl) {
    if ((e = thick_cols_launch<false>(a, X, tab, ph, s))) return e;
    thick_slab(p, sl + 1);
    if ((e = rows(sl + 1 < p.S ? THICK_MIDDLE : THICK_LAST))) return e;
  }
  return THZ_OK;
}

// lanes per map pixel of thick_grad_reduce: about eight terms a lane
static int thick_reduce_lanes(const ThickArgs& a) {
  const long long n = (long long)a.BC * ((a.H + a.hs - 1) / a.hs) * ((a.W + a.ws - 1) / a.ws);
  int g = 1;
  while (g < THICK_REDUCE_THREADS && (long long)g * 8 < n) g *= 2;
  return g;
}
static long long thick_reduce_blocks(const ThickArgs& a) {
  const long long per = THICK_REDUCE_THREADS / thick_reduce_lanes(a);
  return ((long long)a.hs * a.ws + per - 1) / per;
}

// the backward's plan: the forward's, and the partials [BC][H][W] float32 behind its workspace
static int thick_backward_plan(const thz_thick_desc* d, ThickPlan* p, size_t* part) {
  int e = thick_plan(d, p);
  if (e) return e;
  if (thick_reduce_blocks(p->a) > 0x7fffffffLL)
    return fail(THZ_E_UNSUPPORTED, "thick DOE backward: map %dx%d gives more than 2^31 - 1 workgroups", d->hs, d->ws);
  *part = align256((size_t)p->a.BC * d->H * d->W * sizeof(float));
  return THZ_OK;
}

}  // namespace thz

extern "C" int thz_thick_forward(const thz_thick_desc* d, const void* field, const float* height, void* out,
                                 void* workspace, size_t workspace_bytes, thz_stream_t stream) {
  ThickPlan p;
  int e = thick_plan(d, &p);
  if (e) return e;
  if (!field || !height || !out) return fail(THZ_E_ARG, "null data pointer");
  if ((e = check_workspace(workspace, workspace_bytes, p.total()))) return e;
  return thick_forward(d, p, field, height, out, nullptr, workspace, stream);
}

extern "C" int thz_thick_forward_saved(const thz_thick_desc* d, const void* field, const float* height, void* out,
                                       void* stash, void* workspace, size_t workspace_bytes, thz_stream_t stream) {
  ThickPlan p;
  int e = thick_plan(d, &p);
  if (e) return e;
  if (!field || !height || !out || !stash) return fail(THZ_E_ARG, "null data pointer");
  if ((e = check_workspace(workspace, workspace_bytes, p.total()))) return e;
  return thick_forward(d, p, field, height, out, stash, workspace, stream);
}

extern "C" int thz_thick_backward_workspace_size(const thz_thick_desc* d, size_t* bytes) {
  ThickPlan p;
  size_t part;
  int e = thick_backward_plan(d, &p, &part);
  if (e) return e;
  if (!bytes) return fail(THZ_E_ARG, "null bytes");
  *bytes = p.total() + part;
  return THZ_OK;
}

extern "C" int thz_thick_backward(const thz_thick_desc* d, const void* grad_out, const float* height, const void* stash,
                                  void* grad_field, float* grad_height, void* workspace, size_t workspace_bytes,
                                  thz_stream_t stream) {
  ThickPlan p;
  size_t part_bytes;
  int e = thick_backward_plan(d, &p, &part_bytes);
  if (e) return e;
  if (!grad_out || !height) return fail(THZ_E_ARG, "null data pointer");
  if (grad_height && !stash) return fail(THZ_E_ARG, "thick DOE backward: grad_height needs the forward's stash");
  if (!grad_field && !grad_height) return fail(THZ_E_ARG, "thick DOE backward: no gradient asked for");
  if ((e = check_workspace(workspace, workspace_bytes, p.total() + part_bytes))) return e;
  ThickArgs& a = p.a;
  hipStream_t s = (hipStream_t)stream;
  float2* X = (float2*)workspace;
  float2* tab = (float2*)((char*)workspace + p.x);
  float* part = grad_height ? (float*)((char*)workspace + p.total()) : nullptr;
  if ((e = thick_table(d, a, tab, stream))) return e;
  FftPlan pw, ph;
  if ((e = get_plan(a.Pw, &pw)) || (e = get_plan(a.Ph, &ph))) return e;
  auto rows = [&](int mode) {
    KernelTimer kt("thick_grad_rows", s);
    on_thick(a.Pw, [&](auto N) {
      auto k = mode == THICK_FIRST ? thick_grad_rows<N(), THICK_FIRST>
               : mode == THICK_LAST ? thick_grad_rows<N(), THICK_LAST>
                                    : thick_grad_rows<N(), THICK_MIDDLE>;
      hipLaunchKernelGGL(k, dim3(a.BC * a.H), dim3(thick_threads(a.Pw)), thick_lds(a.Pw), s, (const float2*)grad_out,
                         height, X, (const float2*)stash, (float2*)grad_field, part, pw, a);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
    return THZ_OK;
  };
  if ((e = rows(THICK_FIRST))) return e;
  for (int sl = p.S - 1; sl >= 0; --sl) {
    if ((e = thick_cols_launch<true>(a, X, tab, ph, s))) return e;
    thick_slab(p, sl);
    if ((e = rows(sl > 0 ? THICK_MIDDLE : THICK_LAST))) return e;
  }
  if (grad_height) {
    ThickReduceArgs r{a.BC, a.H, a.W, a.hs, a.ws, p.S, thick_reduce_lanes(a), a.dz, p.dz};
    KernelTimer kt("thick_grad_reduce", s);
    hipLaunchKernelGGL(thick_grad_reduce, dim3((unsigned)thick_reduce_blocks(a)), dim3(THICK_REDUCE_THREADS), 0, s,
                       (const float*)part, height, grad_height, r);
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  return THZ_OK;
}
