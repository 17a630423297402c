// Band-limited angular-spectrum propagation (Props/ASM_Prop.py:17-378) for gfx950.
//
// The reference computes crop(ift2(ft2(pad x) * H_centred)).  The four fftshifts cancel
// against the centred grid, so this is crop(IFFT2(FFT2(pad x) * H_nat))
// with H evaluated on the natural (fftfreq) index order.  It runs as three LDS passes
// with NO materialised padding, transfer function or shifts:
//
//   K1 rows_fwd  : per input row, length-Pw FFT of the zero-padded row; keep only the
//                  spectral column band |m_y| <= J that can be non-zero (evanescent and
//                  band-limit cut-offs, computed on the host), store column-major
//                  T[bc][c][h] so the column pass reads contiguous memory.
//   K2 cols      : per (bc, band column c): length-Ph FFT of the zero-padded column,
//                  then for each z of the chunk: x H_z(kx, ky) evaluated on the fly
//                  (fp32, same operation order as the reference, contraction off),
//                  inverse FFT, keep the Ho cropped rows, scale 1/(Ph Pw).  The spectrum
//                  is kept in registers across the z loop (forward FFT once per column).
//   K3 rows_inv  : per output row, gather the band (zero elsewhere), length-Pw inverse
//                  FFT, keep the Wo cropped columns, write out[z][b][c][h][w].
//
// The adjoint (autograd backward) is the same pipeline with conj(H) and the input and
// output windows exchanged.
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <cmath>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_launch.hpp"
#include "thz_wfft.hpp"


namespace thz {

// non-temporal (streaming) 8-byte store
__device__ __forceinline__ void st_stream(float2* p, float2 v) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  __builtin_nontemporal_store(f32x2{v.x, v.y}, reinterpret_cast<f32x2*>(p));
}

constexpr float TWO_PI_F = 6.283185307179586f;  // (float)(2*pi), as torch casts the python scalar

struct AsmArgs {
  int BC, C;
  int Ph, Pw;
  int in_r0, in_c0, Hin, Win;     // input window inside the padded plane
  int out_r0, out_c0, Hout, Wout; // output window
  int ncols, J;                   // kept spectral columns, m_y = c - J
  int ncb;                        // column blocks of CB columns (blocked T layout)
  int ncbu;                       // column blocks of CBU columns (blocked U layout)
  int nz, zoff;                   // z-planes in this chunk, offset into zv
  int kfull, kparts;              // K2 tasks: kfull whole columns, then the rest split in kparts z-ranges
  int bl, adjoint;
  // adjoint over Z planes in one pipeline (autograd backward of a multi-plane forward): K1 runs
  // over the chunk's nz input planes (T holds nz planes), K2 sums FFT(T_z) conj(H_z) over them
  // into one spectrum per column and inverts once (zacc: add into U, for the chunks after the
  // first), K3 runs once on the single summed plane
  int zsum, zacc;
  // 1: the power-of-two column pass may take the plane recurrence where its planes allow it
  // (asm_cols_body decides per column; 0 = THZ_K2_RECURRENCE=0, the per-plane sincos everywhere)
  int zrec;
  float dx, dy, scale;
  const float2* tft;  // RSC: column-major transfer-function table [C][ncols][Ph] (nullptr: analytic ASM)
  int vec;            // VRS: plane b == 2 is Ez = (Ex x + Ey y) / r computed in the row pass
  float zr;           // VRS: z of the Ez grid
  float* sqt;         // mixed-radix K2: sqrt(k^2 - Kx^2 - Ky^2) per [C][ncols][Ph] (asm_tf_tables)
  int* mzt;           // mixed-radix K2: kept-row bound M_z per [C][ncols][nz] of the current z-chunk
  // fused DOE modulation in the row pass (thz_asm_forward_modulated): the input row is field * t_c(h)
  const float* mod_h;   // height map [mod_hs][mod_ws] (nullptr: no modulation)
  const float* mod_u;   // U[0,1) height-noise draw, same shape (nullptr: no noise)
  float* mod_hfull;     // optional: the noisy, upsampled height map [Hin][Win]
  int mod_hs, mod_ws;
  float mod_tol, mod_eps, mod_tand;
  const unsigned* mod_rng;  // device generator state for the height noise when mod_u is null
  unsigned mod_rng_stream;
  // fused |E|^2 -> normalize -> MSE in K3's storer (thz_asm_forward_loss, Z == 1): ls.stats
  // non-null; K1 zeroes its accumulators
  LossSink ls;
  // adjoint of the fused loss (thz_asm_adjoint_loss): the row pass's input is the loss gradient
  // dL/dE at the forward output lg_field (thz_intensity_mse_backward's formula), plus the out
  // cotangent `in` when that is given
  const float2* lg_field;
  const float* lg_gloss;
  const float* lg_target;
  const float* lg_stats;
  int lg_tB, lg_tC;
  float lg_two_inv_n;
  // mixed-radix K2 tables of the first z-chunk computed by tab_blocks extra K1 workgroups
  int tab_blocks;
  // thz_asm_desc.window_mask: 1 = multiply the K3 stores by the mask (forward), 2 = the K1 loads
  // (adjoint input); apm is the mask on that grid
  int ap_side;
  ApertureArgs apm;
  const float* zdev;  // thz_asm_desc.z_dev: the plane distances in device memory (nullptr: zv)
  float lam[THZ_MAX_WAVELENGTHS];
  float zv[THZ_MAX_Z];
};

// plane distance i of the call: from device memory when the caller gave z_dev (graph-replayable)
__device__ __forceinline__ float zval(const AsmArgs& a, int i) { return a.zdev ? a.zdev[i] : a.zv[i]; }


// Per-(wavelength, z) scalars of the transfer function, fp32 with the reference's
// operation order (Props/ASM_Prop.py:253, 290-294, 303-304).
struct TfScalars {
  float z, kl2, A, Bv, kxm, kym;
};

#pragma clang fp contract(off)
__device__ __forceinline__ TfScalars tf_scalars(const AsmArgs& a, float lam, float z) {
  TfScalars s;
  s.z = z;
  const float kl = TWO_PI_F / lam;
  s.kl2 = kl * kl;
  const float du = ((TWO_PI_F / a.dx) / (float)(2 * a.Ph)) / TWO_PI_F;
  const float dv = ((TWO_PI_F / a.dy) / (float)(2 * a.Ph)) / TWO_PI_F;  // Ph for v too (:291)
  const float tu = (2.0f * du) * z;
  const float tv = (2.0f * dv) * z;
  const float ul = (1.0f / sqrtf(tu * tu + 1.0f)) / lam;
  const float vl = (1.0f / sqrtf(tv * tv + 1.0f)) / lam;
  const float au = TWO_PI_F * ul, av = TWO_PI_F * vl;
  s.A = au * au;
  s.Bv = av * av;
  const float lx = (float)a.Ph * a.dx, ly = (float)a.Ph * a.dy;  // length_y uses Ph (:275)
  const float ax = (2.0f * (1.0f / lx)) * z, ay = (2.0f * (1.0f / ly)) * z;
  s.kxm = (TWO_PI_F / sqrtf(ax * ax + 1.0f)) / lam;
  s.kym = (TWO_PI_F / sqrtf(ay * ay + 1.0f)) / lam;
  return s;
}

__device__ __forceinline__ float kfreq(int m, int P, float d) { return (TWO_PI_F * ((float)m / (float)P)) / d; }
// single IEEE operations that must not be fused with neighbours (contraction is off here)
__device__ __forceinline__ float tf_mul(float x, float y) { return x * y; }
__device__ __forceinline__ float tf_add(float x, float y) { return x + y; }
__device__ __forceinline__ float tf_sub(float x, float y) { return x - y; }
__device__ __forceinline__ float tf_div(float x, float y) { return x / y; }



// Mask of H at spectral row m (Kx = kfreq(m)) for the column Ky: exactly the tests of
// tf_value below, in the same fp32 operation order.
__device__ __forceinline__ bool tf_pass(int bl, int Ph, float dx, const TfScalars& s, float Ky, int m) {
  const float Kx = kfreq(m, Ph, dx);
  const float Kx2 = Kx * Kx, Ky2 = Ky * Ky;
  const float d = s.kl2 - (Kx2 + Ky2);
  if (d < 0.0f) return false;
  if (bl == THZ_BANDLIMIT_EXACT) {
    const bool c1 = (Kx2 / s.A + Ky2 / s.kl2) <= 1.0f;
    const bool c2 = (Kx2 / s.kl2 + Ky2 / s.Bv) <= 1.0f;
    return c1 && c2;
  }
  if (bl == THZ_BANDLIMIT_APPROX) return !(fabsf(Kx) > s.kxm || fabsf(Ky) > s.kym);
  return true;
}

// H(kx, ky) = exp(i z sqrt(k^2 - K^2)) with the evanescent and band-limit masks
// (Props/ASM_Prop.py:245-306).  conj for the adjoint.
__device__ __forceinline__ float2 tf_value(const AsmArgs& a, const TfScalars& s, float Kx, float Ky) {
  const float Kx2 = Kx * Kx, Ky2 = Ky * Ky;
  const float K2 = Kx2 + Ky2;
  const float d = s.kl2 - K2;
  if (d < 0.0f) return make_float2(0.f, 0.f);
  if (a.bl == THZ_BANDLIMIT_EXACT) {
    const bool c1 = (Kx2 / s.A + Ky2 / s.kl2) <= 1.0f;
    const bool c2 = (Kx2 / s.kl2 + Ky2 / s.Bv) <= 1.0f;
    if (!(c1 && c2)) return make_float2(0.f, 0.f);
  } else if (a.bl == THZ_BANDLIMIT_APPROX) {
    if (fabsf(Kx) > s.kxm || fabsf(Ky) > s.kym) return make_float2(0.f, 0.f);
  }
  const float ang = s.z * sqrtf(d);
  float sn, cs;
  sincos_rad(ang, &sn, &cs);
  return make_float2(cs, a.adjoint ? -sn : sn);
}
#pragma clang fp contract(on)

// Compile-time mixed-radix sizes (MxPlan, one 64-thread workgroup per transform): the P = 300
// grid of the cfg4 / cfg5 layers.  Other non-power-of-two sizes run the runtime plan.
constexpr int MX_T = 64;
// threads of a compile-time mixed-radix transform: one wave for 300 (the radix-5 stages' 60
// butterflies on one lane each), two waves for 500 (its radix-5 stages' 100 and radix-4 stage's 125
// butterflies one per lane: on one wave, two per lane, the row and column passes spilled)
__host__ __device__ constexpr int mx_threads(int n) { return n == 500 ? 128 : MX_T; }
// waves per SIMD of the mixed-radix column pass: 6 lets it keep its 70 VGPRs (8 spilled 5 of them
// to scratch): cfg5 chained batch 256 0.986 -> 0.952 ms, dual-plane 0.080 -> 0.077 ms per step,
// batch 32 0.290 -> 0.296 (profiles/r05_experiments.txt 4)
constexpr int MX_WPE = 6;
__host__ __device__ constexpr bool is_mx(int n) { return n == Mx300::N || n == Mx500::N; }

__device__ __forceinline__ int band_col(int j, int P, int J, int ncols) {
  const int c = freq_index(j, P) + J;
  return (c >= 0 && c < ncols) ? c : -1;
}

// ---------------------------------------------------------------------------------------------
// K1: row FFT of the zero-padded input rows -> band columns, column-major T[bc][c][h]
// ---------------------------------------------------------------------------------------------
template <int PN>
__device__ __forceinline__ void tf_tables_body(const AsmArgs& a, int blk, int with_sq);
// The K1 input element s of row h of plane `plane` (s < Win): the field, or what the fused
// loaders make of it -- the loss gradient of the adjoint of the fused loss, the DOE modulation
// t_c(h + noise) (writing the noisy height map once), or the VRS Ez plane.
// AP: apply the window mask of the adjoint's input (only the 300-point row pass carries it: the
// runtime test costs the 64-VGPR power-of-two row kernels registers)
template <bool AP>
struct RowSrc {
  const AsmArgs& a;
  const float2* in;
  const float2* src;
  int h, bc;
  bool ez;
  const float2 *sx, *sy;
  float xh;
  int hsrc;
  float lam_c;
  const float2* lg_row = nullptr;
  const float* lg_t = nullptr;
  float lg_m = 0.f, lg_S = 0.f, lg_g = 0.f;
  int lg_am = -1;
  __device__ __forceinline__ RowSrc(const AsmArgs& a_, const float2* in_, int plane, int h_) : a(a_), in(in_), h(h_) {
    bc = plane % a.BC;
    src = in + ((size_t)((a.zsum ? a.zoff * a.BC : 0) + plane) * a.Hin + h) * a.Win;
    // VRS (Props/RSC_Prop.py:294-303): plane b = 2 is Ez = Ex x / r + Ey y / r on the unpadded
    // grid linspace(-N dx/2, N dx/2, N) (dx on both axes, :83-84)
    ez = a.vec && bc / a.C == 2;
    sx = in + ((size_t)(bc % a.C) * a.Hin + h) * a.Win;
    sy = in + ((size_t)(a.C + bc % a.C) * a.Hin + h) * a.Win;
    xh = ez ? lin(-(float)a.Hin * a.dx / 2.0f, (float)a.Hin * a.dx / 2.0f, a.Hin, h) : 0.f;
    hsrc = a.mod_h ? doe_nearest_src(h, a.mod_hs, a.Hin) * a.mod_ws : 0;
    lam_c = a.lam[bc % a.C];
    // loss gradient rows: field E, target T and the statistics of loss item b (the forward's plane
    // z and batch item: b = z B + batch, the Z-summing adjoint's planes included)
    if (a.lg_field) {
      const int gp = (a.zsum ? a.zoff * a.BC : 0) + plane;
      const int b = gp / a.C, c = gp - b * a.C;
      lg_row = a.lg_field + ((size_t)gp * a.Hin + h) * a.Win;
      const int tb = a.lg_tB == 1 ? 0 : b, tc = a.lg_tC == 1 ? 0 : c;
      lg_t = a.lg_target + (((size_t)tb * a.lg_tC + tc) * a.Hin + h) * a.Win;
      lg_m = a.lg_stats[3 * b];
      lg_S = a.lg_stats[3 * b + 2];
      // the argmax relative to this row's first element (c H + h) W
      lg_am = __float_as_int(a.lg_stats[3 * b + 1]) - (c * a.Hin + h) * a.Win;
      lg_g = a.lg_gloss[0] * a.lg_two_inv_n;
    }
  }
  __device__ __forceinline__ float2 operator()(int s) const {
    const float2 v = value(s);
    // the adjoint of (window mask) * ASM: the mask on the adjoint's input (NaN / inf propagate)
    if constexpr (AP) return a.ap_side == 2 && !aperture_open(a.apm, h, s) ? cscale(v, 0.f) : v;
    else return v;
  }
  __device__ __forceinline__ float2 value(int s) const {
    if (a.lg_field) {  // dL/dE = 2 E dL/dI, dL/dI = g (r / m - [argmax] S / m^2) (mse_backward_kernel)
      const float2 e = lg_row[s];
      const float I = loss_intensity(e);
      const float r = I / lg_m - lg_t[s];
      float dI = lg_g * r / lg_m;
      if (s == lg_am) dI -= lg_g * lg_S / (lg_m * lg_m);
      const float2 gl = make_float2(2.f * dI * e.x, 2.f * dI * e.y);
      return in ? cadd(src[s], gl) : gl;
    }
    if (a.mod_h) {  // DOELayer.modulate fused into the loader (Components/QuantizedDOE.py:92-126)
      const float hv = doe_noisy_h(a.mod_h, a.mod_u, hsrc + doe_nearest_src(s, a.mod_ws, a.Win), a.mod_tol,
                                   a.mod_rng, a.mod_rng_stream);
      if (a.mod_hfull && bc == 0) a.mod_hfull[(size_t)h * a.Win + s] = hv;
      return cmul(src[s], doe_transmission(hv, lam_c, a.mod_eps, a.mod_tand, nullptr));
    }
    if (!ez) return src[s];
    return vrs_ez(sx[s], sy[s], xh, lin(-(float)a.Win * a.dx / 2.0f, (float)a.Win * a.dx / 2.0f, a.Win, s), a.zr);
  }
};


// MID (PN = 300 only): the input window [N/3, 2N/3) of the layers' geometry as constants
template <int PN, bool MID = false>
__global__ void __launch_bounds__(1024) THZ_ROW_ATTR asm_rows_fwd(const float2* __restrict__ in, float2* __restrict__ T,
                                                    FftPlan pw, AsmArgs a) {
  static_assert(!MID || is_mx(PN), "window constants: the 300-point pass");
  extern __shared__ float2 lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nrows = gridDim.x - a.tab_blocks;
  if constexpr (PN == Mx300::N) {
    // the extra workgroups past the rows: the mixed-radix column pass's tables of the first
    // z-chunk (asm_tf_tables, one launch fewer; K2 runs after this kernel on the stream).  The
    // 300-point pass only: in asm_rows_fwd<500> the tables' code made the compiler copy the whole
    // argument block to scratch (1.6 KB per lane); P = 500 launches asm_tf_tables<500> instead
    if ((int)blockIdx.x >= nrows) {
      tf_tables_body<PN>(a, blockIdx.x - nrows, 1);
      return;
    }
  }
  const int row = xcd_rows(blockIdx.x, nrows);
  // plane = zz * BC + bc: one plane (zz = 0) except in the Z-summing adjoint, whose chunk's input
  // planes start at plane zoff * BC of `in`
  const int plane = row / a.Hin, h = row - plane * a.Hin;
  float2* dst = T + (size_t)plane * a.ncb * CB * a.Hin;
  const RowSrc<is_mx(PN)> fetch(a, in, plane, h);  // the 300-point pass carries the adjoint's window mask
  if constexpr (PN > 0 && !is_mx(PN)) {
    // twiddle-table loads first, their LDS writes after the row loads (as in K3)
    constexpr int TT = Geo<PN>::T;
    const auto twf = tw_fetch<PN, TT>(pw.tw, tid);
    const TwLds twl = tw_lds_at<PN>(tw_slot<PN>(lds));
    auto tw_hook = [&]() { tw_store<PN, TT>(tw_slot<PN>(lds), twf, tid); };
    auto ld = [&](int, int, int idx) {
      const int s = idx - a.in_c0;
      return (s >= 0 && s < a.Win) ? fetch(s) : make_float2(0.f, 0.f);
    };
    auto sv = [&](int, int, int j, float2 v) {
      const int c = band_col(j, PN, a.J, a.ncols);
      if (c >= 0) dst[blk(c, h, a.Hin)] = v;
    };
    fft_pow2_run<false, PN, TT, FFT_ROWS>(lds, twl, tid, ld, sv, tw_hook);
  } else if constexpr (is_mx(PN)) {
    constexpr int MT = mx_threads(PN);
    if constexpr (MID) __builtin_assume(tid >= 0 && tid < MT);
    using MP = typename MxOf<PN>::type;
    const auto twr = MP::template twiddles<MT>(pw.tw, tid);
    auto ld = [&](int, int, int idx) {
      const int s = idx - (MID ? PN / 3 : a.in_c0);
      return (s >= 0 && s < (MID ? PN / 3 : a.Win)) ? fetch(s) : make_float2(0.f, 0.f);
    };
    auto sv = [&](int, int, int j, float2 v) {
      const int c = band_col(j, PN, a.J, a.ncols);
      if (c >= 0) dst[blk(c, h, a.Hin)] = v;
    };
    MP::template run<false, MT>(lds, twr, tid, ld, sv);
  } else {
    for (int j = tid; j < a.Pw; j += nt) {
      const int s = j - a.in_c0;
      lds[padx(j)] = (s >= 0 && s < a.Win) ? fetch(s) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    fft_lds<false>(lds, pw, tid, nt);
    for (int c = tid; c < a.ncols; c += nt) {
      int j = c - a.J;
      if (j < 0) j += a.Pw;
      dst[blk(c, h, a.Hin)] = lds[padx(j)];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// K2: per band column: FFT(Ph) once, then per z: x H_z, IFFT(Ph), crop, scale -> U[z][bc][c][r]
// ---------------------------------------------------------------------------------------------
// Plane zz of the column task's range [z_lo, z_hi) may be reached from its predecessor in the order
// the planes are run (ascending, or descending from the range's last plane) by the plane recurrence
// of asm_cols_body: with dz the range's first step in that order, the step to zz and eps = step - dz
// are both EXACT fp32 differences (so the recurrence's phase sums to (z_zz - z_first) sq exactly)
// and |eps| k <= 1e-4 rad (so 1 + i eps sq stands for exp(i eps sq) to 5e-9).  Evaluated on the
// device, so a device-resident plane list (thz_asm_desc.z_dev) decides exactly as the host list does.
// register slot of the step factor D of kept spectrum value r (r < 4 or r >= 12): the slots
// [4, 12) of sp, whose values are zero whenever the recurrence runs
__host__ __device__ constexpr int rec_dslot(int r) { return r < 4 ? r + 4 : r - 4; }

// the step from plane zp to plane zc against the range's first step z0 -> z1 (either direction)
__device__ __forceinline__ bool recurrence_step_ok(float z0, float z1, float zp, float zc, float kl) {
  const float dz = z1 - z0, step = zc - zp, eps = step - dz;
  return dz != 0.0f && (double)dz == (double)z1 - (double)z0 && (double)step == (double)zc - (double)zp &&
         (double)eps == (double)step - (double)dz && fabs((double)eps) * (double)kl <= 1e-4;
}

// What H_z is for the power-of-two column kernels (asm_cols, asm_cols_slice, asm_cols_slice_adj)
// and the mixed-radix tables: each piece is written once here, in the fp32 operation order the
// planes carry, so the slice and its adjoint apply the very H the full planes do.

// The column task of this workgroup: the first kfull blocks are whole columns (all nz planes; full
// dispatch rounds of the resident-workgroup count), the last partial round's columns are split
// into kparts z-ranges so that round is short instead of a whole column pass on a few CUs.
__device__ __forceinline__ void k2_task(const AsmArgs& a, int& id, int& z_lo, int& z_hi) {
  z_lo = 0;
  z_hi = a.nz;
  if ((int)blockIdx.x < a.kfull) {
    id = xcd_chunk(blockIdx.x, a.kfull);
  } else {
    const int t = blockIdx.x - a.kfull, part = t % a.kparts;
    id = a.kfull + t / a.kparts;
    z_lo = part * a.nz / a.kparts;
    z_hi = (part + 1) * a.nz / a.kparts;
  }
}

// the column pass's LDS behind the transform image and the twiddles: per plane of the task the
// kept-row bound M_z, the recurrence_votes bits and the z value (k2_lds_bytes on the host)
struct ColLds {
  int *mz, *zok;
  float* zl;
};
template <int PN>
__device__ __forceinline__ ColLds col_lds(float2* lds) {
  int* mz = reinterpret_cast<int*>(lds + lds_floats2(PN) + tw_lds_count(PN));
  return {mz, mz + THZ_MAX_Z, reinterpret_cast<float*>(mz + 2 * THZ_MAX_Z)};
}

// The evanescent and band-limit masks are monotone in |m_x| (every fp32 operation of
// Props/ASM_Prop.py:245-306 is monotone), so the kept rows of the column Ky at the plane of s are
// exactly |m_x| <= M_z: M_z by bisection with the exact reference-order tests, -1 when no row passes.
// P = PN as the caller holds it: a.Ph in the column kernels, the constant in tf_tables_body (with
// a.Ph there asm_rows_fwd<300, true> took 37 VGPRs for 36).
template <int PN>
__device__ __forceinline__ int tf_band_bound(const AsmArgs& a, int P, const TfScalars& s, float Ky) {
  int lo = -1, hi = PN / 2 + 1;
  const int bl = a.bl;
  const float dx = a.dx;
  if (tf_pass(bl, P, dx, s, Ky, 0)) {
    lo = 0;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tf_pass(bl, P, dx, s, Ky, mid)) lo = mid;
      else hi = mid;
    }
  }
  return lo;
}

// Plane q of a range of n planes with the z values zv(0 .. n-1).  Bit 0: q is reached from q - 1 in
// ascending order; bit 1: from q + 1 in descending order (the range's last plane first); bit 2 (on
// plane 0): |z| falls along the range (a sweep towards the aperture).
template <class ZV>
__device__ __forceinline__ int recurrence_votes(ZV zv, int q, int n, float kl) {
  const bool fwd = q == 0 || (n >= 2 && recurrence_step_ok(zv(0), zv(1), zv(q - 1), zv(q), kl));
  const bool bwd = q == n - 1 || (n >= 2 && recurrence_step_ok(zv(n - 1), zv(n - 2), zv(q + 1), zv(q), kl));
  const bool inward = q == 0 && fabsf(zv(n - 1)) < fabsf(zv(0));
  return (fwd ? 1 : 0) | (bwd ? 2 : 0) | (inward ? 4 : 0);
}

// The plane recurrence for a range of n planes (mz, zok: the range's M_z and votes in LDS)?  rec:
// yes; rev: run it from the range's last plane.  One plane per lane, every wave voting on its own
// copy (no loop over the planes per thread, no extra barrier); the votes are wave-uniform.
template <int PN>
__device__ __forceinline__ void recurrence_order(const int* mz, const int* zok, int n, int zrec, bool& rec,
                                                 bool& rev) {
  rec = rev = false;
  if (!zrec || n < 3) return;
  bool okf = true, okr = true, wide = false;
  const int lane = threadIdx.x & 63;
  for (int q0 = 0; q0 < n; q0 += 64) {
    const int q = q0 + lane;
    bool pf = true, pr = true, pw = false;
    if (q < n) {
      // the band may only narrow in the order the planes are run (an element that leaves it is
      // zeroed in the recurrence for good): ascending order for a band that narrows with the plane
      // index (cfg2's increasing z), descending order for one that widens (a decreasing z-sweep)
      const int m = mz[q], mp = q > 0 ? mz[q - 1] : m, zk = zok[q];
      pf = (zk & 1) && m <= mp;
      pr = (zk & 2) && m >= mp;
      pw = m >= PN / 4;  // a kept row with |m_x| >= PN/4: the recurrence keeps the values r < 4, r >= 12 only
    }
    okf = okf && __ballot(!pf) == 0;
    okr = okr && __ballot(!pr) == 0;
    wide = wide || __ballot(pw) != 0;
  }
  rec = (okf || okr) && !wide;
  // a band constant over the range allows both orders: run the range from its plane nearest the
  // aperture, as every column with a changing band of the same sweep does (read wave-uniform: the
  // plane order, and with it every plane index and z of the z loop, stays in scalar registers)
  const int zk0 = __builtin_amdgcn_readfirstlane(zok[0]);
  rev = rec && okr && (!okf || (zk0 & 4));
}

// sqrt(k^2 - Kx^2 - Ky^2) of spectral element i of the column (z-independent)
template <int PN>
__device__ __forceinline__ float col_sq(int i, const AsmArgs& a, float kl2, float Ky2) {
  const float Kx = kfreq(freq_index(i, PN), PN, a.dx);
  return sqrtf(fmaxf(tf_sub(kl2, tf_add(tf_mul(Kx, Kx), Ky2)), 0.0f));
}

// H_z = exp(i z sq) (conj: its conjugate) by the hardware sincos: the per-plane form, and the
// recurrence's anchor on the first plane it runs
__device__ __forceinline__ float2 tf_cis(float z, float sq, bool conj) {
  float sn, cs;
  sincos_hw(tf_mul(z, sq), &sn, &cs);
  return make_float2(cs, conj ? -sn : sn);
}
// the recurrence's step factor D = exp(i dz sq), formed in double and rounded once
__device__ __forceinline__ float2 rec_step_factor(float dz, float sq, bool conj) {
  const float2 d = cis_dd((double)dz * (double)sq);
  return make_float2(d.x, conj ? -d.y : d.y);
}
// g (1 + i th), th = eps sq: the recurrence's correction of a step that is not dz exactly
__device__ __forceinline__ float2 rec_correct(float2 g, float th) {
  return make_float2(fmaf(-th, g.y, g.x), fmaf(th, g.x, g.y));
}
// The recurrence keeps value r (r < 4 or r >= 12) of thread tid, element tid + r PN/16 with
// m_x = tid + r PN/16 (r < 4), tid + r PN/16 - PN (r >= 12), while |m_x| <= Ms
template <int PN>
__device__ __forceinline__ bool rec_keep(int r, int tid, int Ms) {
  return r < 4 ? tid <= Ms - r * (PN / 16) : tid >= PN - r * (PN / 16) - Ms;
}
// slot of kept value r among the eight the slice kernels hold apart (r < 4: 0..3, r >= 12: 4..7)
__host__ __device__ constexpr int rec_kslot(int r) { return r < 4 ? r : r - 8; }
// The per-plane sincos form takes value r of a plane with the kept band M (Ms: its wave-uniform copy)?
// r in [4, 12) are the rows PN/4 <= |m_x| < 3 PN/4: none kept where M < PN/4, skipped on a scalar branch.
template <int PN>
__device__ __forceinline__ bool sincos_keep(int r, int tid, int M, int Ms) {
  if (r >= 4 && r < 12 && Ms < PN / 4) return false;
  const int mx = freq_index(tid + r * (PN / 16), PN);
  return !(mx > M || -mx > M);
}
// exp(2 pi i ((m R) mod PN) / PN) of the slice's row R at element m = tid + r PN/16: m R reduced in
// integers (m, R < 2^14) and the angle in half-turns, both exact, so R = PN / 2 gives exactly +-1
template <int PN>
__device__ __forceinline__ float2 slice_row_phase(int tid, int r, int R) {
  const int k = ((tid + r * (PN / 16)) * R) & (PN - 1);
  float sn, cs;
  sincospif((float)(2 * k) / (float)PN, &sn, &cs);
  return make_float2(cs, sn);
}

// ZSUM: the Z-summing adjoint's column pass (a separate instantiation, so the forward's register
// allocation is untouched by it).
template <int PN, bool ZSUM>
__device__ __forceinline__ void asm_cols_body(const float2* __restrict__ T, float2* __restrict__ U, FftPlan ph,
                                              AsmArgs a) {
  extern __shared__ float2 lds[];
  int id, z_lo, z_hi;
  k2_task(a, id, z_lo, z_hi);
  const int bc = id / a.ncols, c = id - bc * a.ncols;
  const int nt = blockDim.x;
  const int Ph = a.Ph;
  const float2* col = T + (size_t)bc * a.ncb * CB * a.Hin + blk(c, 0, a.Hin);
  const float lam = a.lam[bc % a.C];
  const float Ky = kfreq(c - a.J, a.Pw, a.dy);
  // Each phase works from its own opaque copy of threadIdx.x: otherwise the compiler CSEs /
  // hoists the forward and inverse transforms' LDS addresses and twiddle loads across the
  // whole kernel and spills (the two transforms share every twiddle address).
  int tid = threadIdx.x;
  if constexpr (PN > 0) {
    using S = Pow2Sched<PN>;
    constexpr int TT = Geo<PN>::T;
    // forward = small radix first (its twiddle-free first stage is the cheap one, run once per
    // column); inverse = radix-16 first (twiddle-free, run per z) reading exactly the elements the
    // forward's last radix-16 stage left in this thread's registers
    constexpr int RL = S::radix(S::NST - 1, true);   // radix of the forward's last stage
    constexpr int MBL = PN / RL / TT;                // its butterflies per thread
    float2 sp[MBL][RL];                              // spectrum, element i + r*PN/RL
    const TwLds twl = load_tw_lds<PN>(lds + lds_floats2(PN), ph.tw, threadIdx.x, blockDim.x);
    auto ld0 = [&](int, int, int idx) {
      const int s = idx - a.in_r0;
      return (s >= 0 && s < a.Hin) ? col[(size_t)s * CB] : make_float2(0.f, 0.f);
    };
    auto sv0 = [&](int m, int r, int, float2 v) { sp[m][r] = v; };
    if constexpr (!ZSUM) fft_pow2_io<false, PN, TT, true, false, false>(lds, twl, tid, ld0, sv0);
    if (!ZSUM && !a.tft) {
      // 1 / (Ph Pw) is a power of two: scaling the spectrum once per column instead of every
      // output plane is exact
#pragma unroll
      for (int m = 0; m < MBL; ++m)
#pragma unroll
        for (int r = 0; r < RL; ++r) sp[m][r] = cscale(sp[m][r], a.scale);
    }
    if (!ZSUM && a.tft) {  // RSC: tabulated transfer function FFT2(K), one z
      const float2* tcol = a.tft + ((size_t)(bc % a.C) * a.ncols + c) * PN;
      int tz = threadIdx.x;
      asm volatile("" : "+v"(tz));
      auto ld1 = [&](int m, int r, int idx) {
        const float2 t = tcol[idx];
        return cmul(sp[m][r], a.adjoint ? make_float2(t.x, -t.y) : t);
      };
      float2* dst = U + (size_t)bc * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
      auto sv1 = [&](int, int, int j, float2 v) {
        const int r = j - a.out_r0;
        if (r >= 0 && r < a.Hout) dst[u_roff(r)] = cscale(v, a.scale);
      };
      fft_pow2_io<true, PN, TT, FFT_TAIL, false, false>(lds, twl, tz, ld1, sv1);
      return;
    }
    // One lane per z finds the kept rows |m_x| <= M_z (tf_band_bound); the per-element work is
    // then sqrt once per column and one sincos per z.  zl: the chunk's z values, staged next to
    // mz for the z-loop of the forward (an LDS read per plane instead of a dependent global load
    // at the top of every plane).
    const auto [mz, zok, zl] = col_lds<PN>(lds);
    const float kl = TWO_PI_F / lam;
    const float kl2 = tf_mul(kl, kl);
    const float Ky2 = tf_mul(Ky, Ky);
    // strided over the chunk: a z_chunk may exceed the workgroup (64 threads at P = 1024)
    for (int zz = tid; zz < z_hi - z_lo; zz += nt) {
      const float zq = zval(a, a.zoff + z_lo + zz);
      if constexpr (!ZSUM) zl[zz] = zq;
      mz[zz] = tf_band_bound<PN>(a, a.Ph, tf_scalars(a, lam, zq), Ky);
      if constexpr (!ZSUM)
        zok[zz] = recurrence_votes([&](int q) { return zval(a, a.zoff + z_lo + q); }, zz, z_hi - z_lo, kl);
    }
    // sq of the elements this thread holds, computed once per column
    float sq[MBL][RL];
#pragma unroll
    for (int m = 0; m < MBL; ++m)
#pragma unroll
      for (int r = 0; r < RL; ++r) sq[m][r] = col_sq<PN>(tid + m * TT + r * (PN / RL), a, kl2, Ky2);
    __syncthreads();  // mz visible
    // the plane recurrence (below) for this column?
    bool rec = false, rev = false;
    if constexpr (!ZSUM && RL == 16 && MBL == 1) recurrence_order<PN>(mz, zok, z_hi - z_lo, a.zrec, rec, rev);
    if constexpr (ZSUM) {
      // adjoint over the chunk's planes: sp = sum_z FFT(T_z column) conj(H_z), then one inverse
#pragma unroll
      for (int m = 0; m < MBL; ++m)
#pragma unroll
        for (int r = 0; r < RL; ++r) sp[m][r] = make_float2(0.f, 0.f);
      for (int zz = z_lo; zz < z_hi; ++zz) {
        const float z = zval(a, a.zoff + zz);
        const int M = mz[zz - z_lo];
        const float2* colz = T + ((size_t)zz * a.BC + bc) * a.ncb * CB * a.Hin + blk(c, 0, a.Hin);
        int tz = threadIdx.x;
        asm volatile("" : "+v"(tz));
        auto ldz = [&](int, int, int idx) {
          const int s = idx - a.in_r0;
          return (s >= 0 && s < a.Hin) ? colz[(size_t)s * CB] : make_float2(0.f, 0.f);
        };
        auto acc = [&](int m, int r, int j, float2 v) {
          const int mx = freq_index(j, PN);
          if (mx > M || -mx > M) return;
          float sn, cs;
          sincos_hw(tf_mul(z, sq[m][r]), &sn, &cs);
          sp[m][r] = cadd(sp[m][r], cmul(v, make_float2(cs, -sn)));
        };
        fft_pow2_io<false, PN, TT, true, false, false>(lds, twl, tz, ldz, acc);
      }
#pragma unroll
      for (int m = 0; m < MBL; ++m)
#pragma unroll
        for (int r = 0; r < RL; ++r) sp[m][r] = cscale(sp[m][r], a.scale);
      int tz = threadIdx.x;
      asm volatile("" : "+v"(tz));
      auto ld1 = [&](int m, int r, int) { return sp[m][r]; };
      float2* dst = U + (size_t)bc * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
      auto sv1 = [&](int, int, int j, float2 v) {
        const int r = j - a.out_r0;
        if ((unsigned)r < (unsigned)a.Hout) dst[u_roff(r)] = a.zacc ? cadd(dst[u_roff(r)], v) : v;
      };
      fft_pow2_io<true, PN, TT, FFT_TAIL, false, false>(lds, twl, tz, ld1, sv1);
      return;
    }
    // Plane recurrence (a uniform z-sweep such as cfg2's linspace): instead of one sincos per
    // element per plane, G_j = sp H_{z_j} advances by one complex product per plane,
    //   G_j = G_{j-1} D (1 + i eps_j sq),   D = exp(i dz sq),   eps_j = (z_j - z_{j-1}) - dz,
    // which tracks the given fp32 planes exactly: recurrence_step_ok has checked that every
    // difference is exact in fp32 and |eps_j| k <= 1e-4 rad, so 1 + i theta stands for
    // exp(i theta) to 5e-9.  D is formed in double and rounded once (<= 6e-8 per plane, 4e-6
    // over 64 planes); the first plane run is the sincos form's value bit for bit.  The planes
    // run in the order in which the column's band narrows (ascending z for cfg2; a decreasing
    // sweep runs from the range's last plane), so no element ever re-enters the band.
    // Taken when the column keeps no row with |m_x| >= PN/4 on any plane of the chunk: the
    // inverse's first-stage operands r in [4, 12) are then zero, and the registers of those 8
    // spectrum values hold the 8 step factors D (sp[0][rec_dslot(r)]); sq holds +-sq.  Both forms
    // share one z-loop and one inverse transform on the same registers (as two regions the
    // structurizer kept one form's live-ins live through the other and spilled).
    constexpr bool REC = !ZSUM && RL == 16 && MBL == 1;
    float dz = 0.f, zprev = 0.f;
    int Mprev = -2;  // below every band value (M = -1: no row of the column kept)
    // plane order: ascending, or descending where the recurrence runs the range backwards
    const int zfirst = rev ? z_hi - 1 : z_lo, zstep = rev ? -1 : 1;
    if constexpr (REC) {
      if (rec) {
        const float z0 = zl[zfirst - z_lo];
        dz = zl[zfirst + zstep - z_lo] - z0;
        zprev = z0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (r >= 4 && r < 12) continue;
          sp[0][r] = cmul(sp[0][r], tf_cis(z0, sq[0][r], a.adjoint));
          sp[0][rec_dslot(r)] = rec_step_factor(dz, sq[0][r], a.adjoint);
          if (a.adjoint) sq[0][r] = -sq[0][r];
          // one element's double-precision evaluation at a time (all eight interleaved need more
          // registers than the kernel has)
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    for (int it = 0; it < z_hi - z_lo; ++it) {
      const int zz = zfirst + it * zstep;
      const float z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(zl[zz - z_lo])));
      const int M = mz[zz - z_lo];
      if constexpr (REC) {
        if (rec && it > 0) {
          const float eps = tf_sub(tf_sub(z, zprev), dz);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (r >= 4 && r < 12) continue;
            sp[0][r] = cmul(sp[0][r], sp[0][rec_dslot(r)]);
          }
          // the step correction 1 + i eps sq, skipped on a scalar branch where the step is dz
          // exactly (60 of cfg2's 63 steps), where it would leave every value as it is
          if (__builtin_amdgcn_readfirstlane(__float_as_int(eps)) != 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              if (r >= 4 && r < 12) continue;
              sp[0][r] = rec_correct(sp[0][r], eps * sq[0][r]);  // sq holds -sq for the adjoint
            }
          }
        }
        zprev = z;
      }
      int tz = threadIdx.x;
      asm volatile("" : "+v"(tz));
      const int Ms = __builtin_amdgcn_readfirstlane(M);
      if constexpr (REC) {
        // the band's edge: on the chunk's first plane and wherever the band narrows (a few of
        // cfg2's planes), the elements outside it are zeroed in G itself -- they stay zero through
        // the recurrence's products, and the band never widens again (the eligibility above) --
        // so the loads below need no per-plane mask
        if (rec && Ms != Mprev) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (r >= 4 && r < 12) continue;
            if (!rec_keep<PN>(r, tz, Ms)) sp[0][r] = make_float2(0.f, 0.f);
          }
        }
        Mprev = Ms;
      }
      // the inverse's first stage (radix RL, L = 1) reads exactly the elements this thread
      // holds in sp: multiply by H_z on the fly in the loader
      // the first stage's operands r in [4, 12) are the rows PN/4 <= |m_x| < 3 PN/4: when this
      // plane's kept band M is below PN/4 (all but the few columns near m_y = 0 at cfg2) they are
      // zero for every thread, and a scalar branch skips their sincos and product
      const bool mid0 = Ms < PN / 4;
      // (sincos_keep's two tests, inline: the recurrence's return sits between them)
      auto ld1 = [&](int m, int r, int idx) {
        if (RL == 16 && r >= 4 && r < 12 && mid0) return make_float2(0.f, 0.f);
        if constexpr (REC) {
          if (rec) return sp[0][r];  // out-of-band elements already zero (above)
        }
        const int mx = freq_index(idx, PN);
        if (mx > M || -mx > M) return make_float2(0.f, 0.f);
        return cmul(sp[m][r], tf_cis(z, sq[m][r], a.adjoint));
      };
      float2* dst = U + ((size_t)zz * a.BC + bc) * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
      auto sv1 = [&](int, int, int j, float2 v) {
        const int r = j - a.out_r0;
        // (ordinary stores: the 4 column workgroups of a U block fill its 32-B sectors in the L2;
        // streaming stores here ran K2 4.1 -> 13.8 ms)
        if ((unsigned)r < (unsigned)a.Hout) dst[u_roff(r)] = v;
      };
      // mid0: stage 0 skips the zero operands' half of its butterfly too (both forms; the
      // recurrence's D slots are never read by it); one scalar branch around stage 0 only
      fft_pow2_io<true, PN, TT, FFT_TAIL, false, false>(lds, twl, tz, ld1, sv1, RL == 16 && mid0);
    }
  } else {
    if constexpr (ZSUM) {
      // adjoint over the chunk's planes (see the power-of-two branch)
      float2 acc[FFT_MAXV];
#pragma unroll
      for (int m = 0; m < FFT_MAXV; ++m) acc[m] = make_float2(0.f, 0.f);
      for (int zz = z_lo; zz < z_hi; ++zz) {
        const TfScalars s = tf_scalars(a, lam, zval(a, a.zoff + zz));
        const float2* colz = T + ((size_t)zz * a.BC + bc) * a.ncb * CB * a.Hin + blk(c, 0, a.Hin);
        int tm = threadIdx.x;
        asm volatile("" : "+v"(tm));
        __syncthreads();  // the previous plane's readers are done with lds
        for (int i = tm; i < Ph; i += nt) {
          const int si = i - a.in_r0;
          lds[padx(i)] = (si >= 0 && si < a.Hin) ? colz[(size_t)si * CB] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        fft_lds<false>(lds, ph, tm, nt);
#pragma unroll
        for (int m = 0; m < FFT_MAXV; ++m) {
          const int i = tm + m * nt;
          if (i < Ph) acc[m] = cadd(acc[m], cmul(lds[padx(i)], tf_value(a, s, kfreq(freq_index(i, Ph), Ph, a.dx), Ky)));
        }
      }
      int tm = threadIdx.x;
      asm volatile("" : "+v"(tm));
      __syncthreads();
#pragma unroll
      for (int m = 0; m < FFT_MAXV; ++m) {
        const int i = tm + m * nt;
        if (i < Ph) lds[padx(i)] = acc[m];
      }
      __syncthreads();
      fft_lds<true>(lds, ph, tm, nt);
      float2* dst = U + (size_t)bc * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
      for (int r = tm; r < a.Hout; r += nt) {
        const float2 v = cscale(lds[padx(a.out_r0 + r)], a.scale);
        dst[u_roff(r)] = a.zacc ? cadd(dst[u_roff(r)], v) : v;
      }
      return;
    }
    for (int i = tid; i < Ph; i += nt) {
      const int s = i - a.in_r0;
      lds[padx(i)] = (s >= 0 && s < a.Hin) ? col[(size_t)s * CB] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    fft_lds<false>(lds, ph, tid, nt);
    float2 sp[FFT_MAXV];
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (int m = 0; m < FFT_MAXV; ++m) {
      const int i = tid + m * nt;
      sp[m] = i < Ph ? lds[padx(i)] : make_float2(0.f, 0.f);
    }
    const float2* tcol = a.tft ? a.tft + ((size_t)(bc % a.C) * a.ncols + c) * Ph : nullptr;
    for (int zz = z_lo; zz < z_hi; ++zz) {
      const TfScalars s = tf_scalars(a, lam, zval(a, a.zoff + zz));
      int tm = threadIdx.x;
      asm volatile("" : "+v"(tm));
      __syncthreads();  // previous z's readers are done with lds
#pragma unroll
      for (int m = 0; m < FFT_MAXV; ++m) {
        const int i = tm + m * nt;
        if (i < Ph)
          lds[padx(i)] = cmul(sp[m], tcol ? (a.adjoint ? make_float2(tcol[i].x, -tcol[i].y) : tcol[i])
                                          : tf_value(a, s, kfreq(freq_index(i, Ph), Ph, a.dx), Ky));
      }
      __syncthreads();
      fft_lds<true>(lds, ph, tm, nt);
      float2* dst = U + ((size_t)zz * a.BC + bc) * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
      for (int r = tm; r < a.Hout; r += nt) dst[u_roff(r)] = cscale(lds[padx(a.out_r0 + r)], a.scale);
    }
  }
}

template <int PN>
__global__ void __launch_bounds__(1024) asm_cols(const float2* __restrict__ T, float2* __restrict__ U, FftPlan ph,
                                                AsmArgs a) {
  asm_cols_body<PN, false>(T, U, ph, a);
}

template <int PN>
__global__ void __launch_bounds__(1024) asm_cols_zsum(const float2* __restrict__ T, float2* __restrict__ U,
                                                     FftPlan ph, AsmArgs a) {
  asm_cols_body<PN, true>(T, U, ph, a);
}

// Per (wavelength, band column) of a mixed-radix Ph: sqrt(k^2 - Kx^2 - Ky^2) of every row
// (z-independent, written on the first z-chunk) and the kept-row bound M_z of each z of the
// chunk (bisection with the exact reference-order tests, one lane per z; see asm_cols).  Every
// plane of the wavelength shares them, so the column pass does no fp32 division.
template <int PN>
__device__ __forceinline__ void tf_tables_body(const AsmArgs& a, int blk, int with_sq) {
  const int li = blk / a.ncols, c = blk - li * a.ncols;
  const float lam = a.lam[li];
  const float Ky = kfreq(c - a.J, a.Pw, a.dy);
  const size_t col = (size_t)li * a.ncols + c;
  if (with_sq) {
    const float kl = TWO_PI_F / lam;
    const float kl2 = tf_mul(kl, kl);
    const float Ky2 = tf_mul(Ky, Ky);
    for (int i = threadIdx.x; i < PN; i += blockDim.x) a.sqt[col * PN + i] = col_sq<PN>(i, a, kl2, Ky2);
  }
  if (a.nz <= 2) {
    // few planes (the DONN / QAT layers: one): every lane tests ceil((PN/2+1)/64) rows and M_z + 1
    // is the number that pass (the kept set is a prefix of |m_x|), instead of one lane's serial
    // bisection
    for (int zz = 0; zz < a.nz; ++zz) {
      const TfScalars s = tf_scalars(a, lam, zval(a, a.zoff + zz));
      int n = 0;
#pragma unroll
      for (int m0 = 0; m0 <= PN / 2; m0 += MX_T) {
        const int m = m0 + (int)threadIdx.x;
        n += __popcll(__ballot(m <= PN / 2 && tf_pass(a.bl, PN, a.dx, s, Ky, m)));
      }
      if (threadIdx.x == 0) a.mzt[col * a.nz + zz] = n - 1;
    }
    return;
  }
  for (int zz = threadIdx.x; zz < a.nz; zz += blockDim.x)
    a.mzt[col * a.nz + zz] = tf_band_bound<PN>(a, PN, tf_scalars(a, lam, zval(a, a.zoff + zz)), Ky);
}

template <int PN>
__global__ void __launch_bounds__(MX_T) asm_tf_tables(AsmArgs a, int with_sq) {
  tf_tables_body<PN>(a, blockIdx.x, with_sq);
}

// K2 for a compile-time mixed-radix Ph (MxPlan, blockDim MX_T): the power-of-two kernel's
// structure -- spectrum kept in registers, H_z applied in the inverse's loader from the
// per-column sqrt and the bisected |m_x| bound, cropped rows stored from the last stage -- with
// the runtime plan's numerics at the output (1 / (Ph Pw) is not a power of two here, so the
// scale is applied to each output element as asm_cols<0> does).
// MID: the 300-point layers' windows ([N/3, 2N/3) in and out: padding 2 with unpad, cfg4 / cfg5)
// as compile-time constants (asm_cols_mx_mid, the default for that geometry)
template <class MP, bool ZSUM, bool MID = false>
__device__ __forceinline__ void asm_cols_mx_body(const float2* __restrict__ T, float2* __restrict__ U, FftPlan ph,
                                                 AsmArgs a) {
  constexpr int PN = MP::N, RL = MP::RL, MT = mx_threads(PN), NBL = PN / RL, MBL = (NBL + MT - 1) / MT;
  static_assert(MP::R0 == RL, "the inverse must start where the forward ends");
  extern __shared__ float2 lds[];
  int id, z_lo, z_hi;
  k2_task(a, id, z_lo, z_hi);
  const int bc = id / a.ncols, c = id - bc * a.ncols;
  const float2* col = T + (size_t)bc * a.ncb * CB * a.Hin + blk(c, 0, a.Hin);
  int tid = threadIdx.x;
  float2 sp[MBL][RL];
  if constexpr (MID) __builtin_assume(tid >= 0 && tid < MT);
  auto ld0 = [&](int, int, int idx) {
    const int s = idx - (MID ? PN / 3 : a.in_r0);
    return (s >= 0 && s < (MID ? PN / 3 : a.Hin)) ? col[(size_t)s * CB] : make_float2(0.f, 0.f);
  };
  auto sv0 = [&](int m, int r, int, float2 v) { sp[m][r] = v; };
  const auto twr = MP::template twiddles<MT>(ph.tw, tid);
  if constexpr (!ZSUM) MP::template run<false, MT>(lds, twr, tid, ld0, sv0);
  if (!ZSUM && a.tft) {  // RSC: tabulated transfer function FFT2(K), one z
    const float2* tcol = a.tft + ((size_t)(bc % a.C) * a.ncols + c) * PN;
    int tz = threadIdx.x;
    asm volatile("" : "+v"(tz));
    auto ld1 = [&](int m, int r, int idx) {
      const float2 t = tcol[idx];
      return cmul(sp[m][r], a.adjoint ? make_float2(t.x, -t.y) : t);
    };
    float2* dst = U + (size_t)bc * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
    auto sv1 = [&](int, int, int j, float2 v) {
      const int r = j - a.out_r0;
      if (r >= 0 && r < a.Hout) dst[u_roff(r)] = cscale(v, a.scale);
    };
    MP::template run<true, MT>(lds, twr, tz, ld1, sv1);
    return;
  }
  // kept rows |m_x| <= M_z per z and the z-independent sqrt(k^2 - K^2) of the elements this
  // thread holds: the wavelength's per-column tables (asm_tf_tables)
  const size_t tc = (size_t)(bc % a.C) * a.ncols + c;
  const int* mzc = a.mzt + tc * a.nz;
  const float* sqc = a.sqt + tc * PN;
  float sq[MBL][RL];
#pragma unroll
  for (int m = 0; m < MBL; ++m) {
    const int i = tid + m * MT;
#pragma unroll
    for (int r = 0; r < RL; ++r) sq[m][r] = (NBL % MT == 0 || i < NBL) ? sqc[i + r * NBL] : 0.f;
  }
  if constexpr (ZSUM) {
    // adjoint over the chunk's planes: sp = sum_z FFT(T_z column) conj(H_z), then one inverse
#pragma unroll
    for (int m = 0; m < MBL; ++m)
#pragma unroll
      for (int r = 0; r < RL; ++r) sp[m][r] = make_float2(0.f, 0.f);
    for (int zz = z_lo; zz < z_hi; ++zz) {
      const float z = zval(a, a.zoff + zz);
      const int M = mzc[zz];
      const float2* colz = T + ((size_t)zz * a.BC + bc) * a.ncb * CB * a.Hin + blk(c, 0, a.Hin);
      int tz = threadIdx.x;
      asm volatile("" : "+v"(tz));
      auto ldz = [&](int, int, int idx) {
        const int s = idx - a.in_r0;
        return (s >= 0 && s < a.Hin) ? colz[(size_t)s * CB] : make_float2(0.f, 0.f);
      };
      auto acc = [&](int m, int r, int j, float2 v) {
        const int mx = freq_index(j, PN);
        if (mx > M || -mx > M) return;
        float sn, cs;
        sincos_hw(tf_mul(z, sq[m][r]), &sn, &cs);
        sp[m][r] = cadd(sp[m][r], cmul(v, make_float2(cs, -sn)));
      };
      MP::template run<false, MT>(lds, twr, tz, ldz, acc);
    }
    int tz = threadIdx.x;
    asm volatile("" : "+v"(tz));
    auto ld1 = [&](int m, int r, int) { return sp[m][r]; };
    float2* dst = U + (size_t)bc * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
    auto sv1 = [&](int, int, int j, float2 v) {
      const int r = j - a.out_r0;
      if ((unsigned)r < (unsigned)a.Hout) {
        const float2 o = cscale(v, a.scale);
        dst[u_roff(r)] = a.zacc ? cadd(dst[u_roff(r)], o) : o;
      }
    };
    MP::template run<true, MT>(lds, twr, tz, ld1, sv1);
    return;
  }
  for (int zz = z_lo; zz < z_hi; ++zz) {
    const float z = zval(a, a.zoff + zz);
    const int M = mzc[zz];
    int tz = threadIdx.x;
    asm volatile("" : "+v"(tz));
    if constexpr (MID) __builtin_assume(tz >= 0 && tz < MT);
    auto ld1 = [&](int m, int r, int idx) {
      const int mx = freq_index(idx, PN);
      if (mx > M || -mx > M) return make_float2(0.f, 0.f);
      float sn, cs;
      sincos_hw(tf_mul(z, sq[m][r]), &sn, &cs);
      return cmul(sp[m][r], make_float2(cs, a.adjoint ? -sn : sn));
    };
    float2* dst = U + ((size_t)zz * a.BC + bc) * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
    auto sv1 = [&](int, int, int j, float2 v) {
      const int r = j - (MID ? PN / 3 : a.out_r0);
      if ((unsigned)r < (unsigned)(MID ? PN / 3 : a.Hout)) dst[u_roff(r)] = cscale(v, a.scale);
    };
    MP::template run<true, MT>(lds, twr, tz, ld1, sv1);
  }
}

template <class MP>
__global__ void __launch_bounds__(mx_threads(MP::N)) __attribute__((amdgpu_waves_per_eu(MX_WPE))) asm_cols_mx(
    const float2* __restrict__ T, float2* __restrict__ U, FftPlan ph, AsmArgs a) {
  asm_cols_mx_body<MP, false>(T, U, ph, a);
}

template <class MP>
__global__ void __launch_bounds__(mx_threads(MP::N)) __attribute__((amdgpu_waves_per_eu(MX_WPE))) asm_cols_mx_mid(
    const float2* __restrict__ T, float2* __restrict__ U, FftPlan ph, AsmArgs a) {
  asm_cols_mx_body<MP, false, true>(T, U, ph, a);
}

template <class MP>
__global__ void __launch_bounds__(mx_threads(MP::N)) __attribute__((amdgpu_waves_per_eu(MX_WPE))) asm_cols_mx_zsum(
    const float2* __restrict__ T, float2* __restrict__ U, FftPlan ph, AsmArgs a) {
  asm_cols_mx_body<MP, true>(T, U, ph, a);
}

// ---------------------------------------------------------------------------------------------
// K3: per output row: gather band from U, IFFT(Pw), crop -> out[z][bc][r][w]
// ---------------------------------------------------------------------------------------------
// LOSS: the stored row also feeds the |E|^2 -> normalize -> MSE sums of its batch item
// (LossAcc; Z == 1 so plane == bc), stored per workgroup in slot (c, r) of b by loss_store_part.
// MID: the crop as a compile-time window: the middle half of the padded row for the power-of-two
// sizes (out_c0 = PN / 4, Wout = PN / 2: padding scale 1 with unpad, cfg2), the middle third for
// the 300-point layers (out_c0 = Wout = 100: padding 2 with unpad, cfg4 / cfg5)
template <int PN, bool LOSS, bool MID = false>
__device__ __forceinline__ void rows_inv_body(const float2* __restrict__ U, float2* __restrict__ out, FftPlan pw,
                                              const AsmArgs& a) {
  extern __shared__ float2 lds[];
  const int row = xcd_rows(blockIdx.x, gridDim.x);  // row in [0, nz*BC*Hout)
  const int plane = row / a.Hout, r = row - plane * a.Hout;  // plane = zz*BC + bc
  const int tid = threadIdx.x, nt = blockDim.x;
  const float2* src = U + (size_t)plane * a.ncbu * CBU * u_rows(a.Hout);
  float2* dst = out + ((size_t)(a.zoff * a.BC + plane) * a.Hout + r) * a.Wout;
  LossAcc acc;
  const float* trow = nullptr;
  unsigned ibase = 0;
  int lb = 0, lc = 0;
  if constexpr (LOSS) {  // loss item lb = z B + b of the chunk's global plane
    const int gp = a.zoff * a.BC + plane;
    lb = gp / a.C;
    lc = gp - lb * a.C;
    const int tb = a.ls.tB == 1 ? 0 : lb, tc = a.ls.tC == 1 ? 0 : lc;
    trow = a.ls.target + (((size_t)tb * a.ls.tC + tc) * a.Hout + r) * a.Wout;
    ibase = (unsigned)((lc * a.Hout + r) * a.Wout);
  }
  auto put = [&](int w, float2 v) {
    // the window mask of a folded aperture (forward): the 300-point pass only
    if constexpr (is_mx(PN)) if (a.ap_side == 1 && !aperture_open(a.apm, r, w)) v = cscale(v, 0.f);
    if constexpr (PN >= 1024 && !is_mx(PN)) {
      // large planes: written once and not read back by this pipeline, so streaming (non-temporal)
      // stores that do not displace the U lines the neighbouring rows' workgroups still gather
      // (cfg2: K3 4.71 -> 4.45 ms).  The small P = 300 layers' outputs feed the next layer from L2.
      st_stream(dst + w, v);
    } else {
      dst[w] = v;
    }
    if constexpr (LOSS) acc.add(v, trow[w], ibase + (unsigned)w);
  };
  if constexpr (is_mx(PN)) {
    constexpr int MT = mx_threads(PN);
    if constexpr (MID) __builtin_assume(tid >= 0 && tid < MT);
    using MP = typename MxOf<PN>::type;
    const auto twr = MP::template twiddles<MT>(pw.tw, tid);
    auto ld = [&](int, int, int j) {
      const int c = band_col(j, PN, a.J, a.ncols);
      return c >= 0 ? src[blk_u(c, r, a.Hout)] : make_float2(0.f, 0.f);
    };
    // (MID: the layers' output window [N/3, 2N/3))
    auto sv = [&](int, int, int j, float2 v) {
      const int w = j - (MID ? PN / 3 : a.out_c0);
      if ((unsigned)w < (unsigned)(MID ? PN / 3 : a.Wout)) put(w, v);
    };
    MP::template run<true, MT>(lds, twr, tid, ld, sv);
  } else if constexpr (PN > 0) {
    // The twiddle tables' global loads go out first and their LDS writes happen after the first
    // stage's gather (the hook runs before the first exchange), so the gather does not wait behind
    // them: cfg2 K3 4.40 -> 4.28 ms (profiles/r03_k3_probes.txt)
    constexpr int TT = Geo<PN>::T;
    __builtin_assume(tid >= 0 && tid < TT);  // the launch's block size: lets the crop test fold (MID)
    const auto twf = tw_fetch<PN, TT>(pw.tw, tid);
    const TwLds twl = tw_lds_at<PN>(tw_slot<PN>(lds));
    auto tw_hook = [&]() { tw_store<PN, TT>(tw_slot<PN>(lds), twf, tid); };
    // First stage (radix 16, L = 1) reads j = i + q*NB0, i < NB0.  Its band column is
    // c = c0 + delta_q with c0 = i + J >= 0 and delta_q = q*NB0 (- PN for the negative
    // frequencies), a multiple of CBU: the blocked address is then base(c0) + delta_q*Hout,
    // one add per element instead of the full blk_u() per element.
    constexpr int NB0 = PN / pow2_v(PN);  // first stage: radix pow2_v, L = 1
    static_assert(NB0 % CBU == 0, "band offsets must be whole U blocks");
    static_assert(Geo<PN>::T == NB0, "one first-stage butterfly per thread: i = tid");
    const int c0 = tid + a.J;
    const float2* base = src + blk_u(c0, r, a.Hout);
    const long cstride = u_rows(a.Hout);  // blk_u(c + delta) - blk_u(c) = delta * cstride for CBU | delta
    // operands q in [4, 12) are the columns PN/4 <= |m_y| < 3 PN/4: outside the band for every
    // lane of most waves (all but the first and last at cfg2), which then skip their address math
    // and masked loads on one scalar branch
    static_assert(NB0 == PN / 16, "radix-16 first stage");
    const bool mid0 = __all(c0 + 4 * NB0 >= a.ncols && c0 + 11 * NB0 - PN < 0);
    auto ld = [&](int, int q, int) {
      if (q >= 4 && q < 12 && mid0) return make_float2(0.f, 0.f);
      const int delta = q * NB0 >= PN / 2 ? q * NB0 - PN : q * NB0;
      if ((unsigned)(c0 + delta) >= (unsigned)a.ncols) return make_float2(0.f, 0.f);
      return base[(long)delta * cstride];
    };
    auto sv = [&](int, int, int j, float2 v) {
      const int w = j - (MID ? PN / 4 : a.out_c0);
      if ((unsigned)w < (unsigned)(MID ? PN / 2 : a.Wout)) put(w, v);
    };
    // (the stage itself stays the full butterfly on those zeros: dft16's MID_IN form, which the column
    // pass takes on its own mid0, ran this gather-latency-bound pass 4.250 -> 4.300 ms at cfg2 with 32
    // VALU fewer per thread)
    fft_pow2_run<true, PN, TT, FFT_ROWS>(lds, twl, tid, ld, sv, tw_hook);
  } else {
    for (int j = tid; j < a.Pw; j += nt) {
      const int c = band_col(j, a.Pw, a.J, a.ncols);
      lds[padx(j)] = c >= 0 ? src[blk_u(c, r, a.Hout)] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    fft_lds<true>(lds, pw, tid, nt);
    for (int w = tid; w < a.Wout; w += nt) put(w, lds[padx(a.out_c0 + w)]);
  }
  // C Hout slots per item; loss_finish_kernel reduces them (an in-kernel finish by the last
  // workgroup of each item cost one agent-scope release fence -- an L2 writeback -- per workgroup:
  // cfg5 chained 1.10 -> 2.12 ms at batch 256, profiles/r05_experiments.txt)
  if constexpr (LOSS) loss_store_part(acc, a.ls, lb, lc * a.Hout + r);
}

template <int PN>
__global__ void __launch_bounds__(1024) THZ_ROW_ATTR asm_rows_inv(const float2* __restrict__ U, float2* __restrict__ out,
                                                    FftPlan pw, AsmArgs a) {
  rows_inv_body<PN, false>(U, out, pw, a);
}

template <int PN>
__global__ void __launch_bounds__(1024) THZ_ROW_ATTR asm_rows_inv_mid(const float2* __restrict__ U,
                                                                      float2* __restrict__ out, FftPlan pw, AsmArgs a) {
  rows_inv_body<PN, false, true>(U, out, pw, a);
}

template <int PN>
__global__ void __launch_bounds__(1024) THZ_ROW_ATTR asm_rows_inv_loss_mid(const float2* __restrict__ U,
                                                                           float2* __restrict__ out, FftPlan pw,
                                                                           AsmArgs a) {
  rows_inv_body<PN, true, true>(U, out, pw, a);
}

template <int PN>
__global__ void __launch_bounds__(1024) THZ_ROW_ATTR asm_rows_inv_loss(const float2* __restrict__ U,
                                                                       float2* __restrict__ out, FftPlan pw, AsmArgs a) {
  rows_inv_body<PN, true>(U, out, pw, a);
}

// K3 on row pairs (power-of-two sizes, no loss sums): one workgroup runs rows 2i and 2i + 1 of one
// plane through the two-line transform (fft_pow2_run2), so the band tests, the gather and store
// address math, every twiddle read, the table fill and the barriers are paid once per pair.  Both
// rows lie in one 4-row U tile: the pair of a column is 16 contiguous, 16-B aligned bytes and comes
// in one load.  The last workgroup of a plane with an odd Hout has one row: its line 1 transforms
// zeros and stores nothing (a workgroup-uniform select at the loads and the stores; every thread
// runs every barrier).  Each row's arithmetic is rows_inv_body's, bit for bit.
template <int PN, bool MID>
__device__ __forceinline__ void rows_inv_pair_body(const float2* __restrict__ U, float2* __restrict__ out, FftPlan pw,
                                                   const AsmArgs& a) {
  static_assert(PN >= 1024 && !is_mx(PN), "power-of-two sizes");
  static_assert(URT % 2 == 0, "rows 2i and 2i + 1 share a U tile");
  extern __shared__ float2 lds[];
  constexpr int TT = Geo<PN>::T;
  const int hp = (a.Hout + 1) >> 1;                    // row pairs per plane
  const int pr = xcd_rows(blockIdx.x, gridDim.x);      // pair in [0, nz*BC*hp)
  const int plane = pr / hp, r = 2 * (pr - plane * hp);  // plane = zz*BC + bc
  const bool two = r + 1 < a.Hout;                     // workgroup-uniform
  const int tid = threadIdx.x;
  __builtin_assume(tid >= 0 && tid < TT);
  const float2* src = U + (size_t)plane * a.ncbu * CBU * u_rows(a.Hout);
  float2* dst0 = out + ((size_t)(a.zoff * a.BC + plane) * a.Hout + r) * a.Wout;
  float2* dst1 = dst0 + a.Wout;
  const auto twf = tw_fetch<PN, TT>(pw.tw, tid);
  const TwLds twl = tw_lds_at<PN>(tw_slot2<PN>(lds));
  auto tw_hook = [&]() { tw_store<PN, TT>(tw_slot2<PN>(lds), twf, tid); };
  // the gather of rows_inv_body; row r is even, so (r, r + 1) of a column are one aligned float4
  // (u_rows rounds U's rows up to whole tiles before it adds its stride pad: row r + 1 of the one-row
  // tail lies in the tile of row r, so the load stays inside the column's block, short of the pad)
  constexpr int NB0 = PN / pow2_v(PN);
  static_assert(NB0 % CBU == 0, "band offsets must be whole U blocks");
  static_assert(Geo<PN>::T == NB0 && NB0 == PN / 16, "radix-16 first stage, one butterfly per thread");
  const int c0 = tid + a.J;
  const float2* base = src + blk_u(c0, r, a.Hout);
  const long cstride = u_rows(a.Hout);
  const bool mid0 = __all(c0 + 4 * NB0 >= a.ncols && c0 + 11 * NB0 - PN < 0);
  auto ld = [&](int, int q, int, float2& x0, float2& x1) {
    x0 = x1 = make_float2(0.f, 0.f);
    if (q >= 4 && q < 12 && mid0) return;
    const int delta = q * NB0 >= PN / 2 ? q * NB0 - PN : q * NB0;
    if ((unsigned)(c0 + delta) >= (unsigned)a.ncols) return;
    const float4 x = *reinterpret_cast<const float4*>(base + (long)delta * cstride);
    x0 = make_float2(x.x, x.y);
    if (two) x1 = make_float2(x.z, x.w);
  };
  auto sv = [&](int line, int, int, int j, float2 v) {
    const int w = j - (MID ? PN / 4 : a.out_c0);
    if ((unsigned)w < (unsigned)(MID ? PN / 2 : a.Wout) && (line == 0 || two)) st_stream((line ? dst1 : dst0) + w, v);
  };
  fft_pow2_run2<true, PN, TT, FFT_ROWS>(lds, twl, tid, ld, sv, tw_hook);
}

// 4 waves / SIMD: 128 VGPRs for the two lines; at 8192 points two 8-wave workgroups per CU.  (The
// 4096-point schedule 16 16 16 ends in a full radix-16 stage whose twiddles spill at 128: 3 there.)
constexpr int pair_waves_per_eu(int n) { return n == 4096 ? 3 : 4; }
template <int PN, bool MID>
__global__ void __launch_bounds__(Geo<PN>::T) __attribute__((amdgpu_waves_per_eu(pair_waves_per_eu(PN))))
asm_rows_inv_pair(const float2* __restrict__ U, float2* __restrict__ out, FftPlan pw, AsmArgs a) {
  rows_inv_pair_body<PN, MID>(U, out, pw, a);
}

// ---------------------------------------------------------------------------------------------
// z-x slice (thz_asm_slice_forward): one output row of every plane of a z-sweep
// (experiment_extend_depth_of_focus.ipynb:229-263 keeps final_field.data[0, 0, 49, :] per z).
// For the padded-plane row R = row + out_r0,
//   U_z[c][R] = (1 / Ph) sum_m S_c[m] H_z(m, c) exp(+2 pi i m R / Ph),
// S_c the column spectrum the column pass holds in registers: the z-independent phase is folded into
// S_c once, and a plane then costs the transfer-function product and a sum -- no inverse column
// transform, no LDS exchange, no barrier and no U store per plane.
//   K2s cols_slice: per (bc, band column): FFT(Ph) once, x scale exp(2 pi i m R / Ph), then per z of
//                   the chunk sum_m S'[m] H_z(m) -> V[z][bc][c]
//   K3s rows_slice: per (z, bc): gather the band from V, IFFT(Pw), crop -> out[z][bc][w]
// ---------------------------------------------------------------------------------------------
// planes per cols_slice launch: the plane recurrence restarts with every launch, and its error
// budget (D rounded once, 6e-8 per plane) is stated for 64 planes
constexpr int SLICE_ZC = 64;

// The transfer-function side is asm_cols_body's forward (ZSUM = false, a.tft = nullptr) through the
// same helpers (k2_task, tf_band_bound, recurrence_votes, recurrence_order, col_sq, tf_cis,
// rec_step_factor, rec_correct, rec_keep), on the same tasks and z-chunks -- so every plane's H
// carries the very rounding it has in asm_cols, and the slice differs from the full planes' row by
// the summation alone.  Not shared: where the step factors live (dstep here, the spectrum's free
// slots in asm_cols_body) and the z loop around them, which each kernel's register allocation shapes.
template <int PN>
__global__ void __launch_bounds__(1024) asm_cols_slice(const float2* __restrict__ T, float2* __restrict__ V,
                                                      FftPlan ph, AsmArgs a, int R) {
  extern __shared__ float2 lds[];
  using S = Pow2Sched<PN>;
  constexpr int TT = Geo<PN>::T;
  static_assert(S::radix(S::NST - 1, true) == 16 && PN / 16 / TT == 1, "one radix-16 butterfly per thread");
  int id, z_lo, z_hi;
  k2_task(a, id, z_lo, z_hi);
  const int bc = id / a.ncols, c = id - bc * a.ncols;
  const int nt = blockDim.x, nz = z_hi - z_lo;  // this task's planes: z_lo + [0, nz) of the chunk
  const float2* col = T + (size_t)bc * a.ncb * CB * a.Hin + blk(c, 0, a.Hin);
  const float lam = a.lam[bc % a.C];
  const float Ky = kfreq(c - a.J, a.Pw, a.dy);
  const int tid = threadIdx.x;
  float2 sp[16];  // spectrum, element tid + r PN/16
  const TwLds twl = load_tw_lds<PN>(lds + lds_floats2(PN), ph.tw, threadIdx.x, blockDim.x);
  auto ld0 = [&](int, int, int idx) {
    const int s = idx - a.in_r0;
    return (s >= 0 && s < a.Hin) ? col[(size_t)s * CB] : make_float2(0.f, 0.f);
  };
  auto sv0 = [&](int, int r, int, float2 v) { sp[r] = v; };
  fft_pow2_io<false, PN, TT, true, false, false>(lds, twl, tid, ld0, sv0);
  // S'[m] = S[m] / (Ph Pw) exp(2 pi i ((m R) mod Ph) / Ph)
#pragma unroll
  for (int r = 0; r < 16; ++r) sp[r] = cmul(cscale(sp[r], a.scale), slice_row_phase<PN>(tid, r, R));
  const auto [mz, zok, zl] = col_lds<PN>(lds);
  const float kl = TWO_PI_F / lam;
  const float kl2 = tf_mul(kl, kl);
  const float Ky2 = tf_mul(Ky, Ky);
  for (int zz = tid; zz < nz; zz += nt) {
    const float zq = zval(a, a.zoff + z_lo + zz);
    zl[zz] = zq;
    mz[zz] = tf_band_bound<PN>(a, a.Ph, tf_scalars(a, lam, zq), Ky);
    zok[zz] = recurrence_votes([&](int q) { return zval(a, a.zoff + z_lo + q); }, zz, nz, kl);
  }
  float sq[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) sq[r] = col_sq<PN>(tid + r * (PN / 16), a, kl2, Ky2);
  __syncthreads();  // mz, zok, zl visible; every wave is done with the transform's LDS image
  bool rec, rev;
  recurrence_order<PN>(mz, zok, nz, a.zrec, rec, rev);
  const int lane = threadIdx.x & 63;
  // each wave's partial sum of plane zz in slot [zz][wave] of the (now free) transform image;
  // the planes are finished after the loop in a fixed order (no barrier inside the z loop)
  float2* part = lds;
  const int wave = threadIdx.x >> 6, nw = nt >> 6;
  float2 dstep[8];  // the step factors D of the kept values r < 4 (slots 0..3) and r >= 12 (4..7)
  float dz = 0.f, zprev = 0.f;
  int Mprev = -2;
  const int zfirst = rev ? nz - 1 : 0, zstep = rev ? -1 : 1;
  if (rec) {
    const float z0 = zl[zfirst];
    dz = zl[zfirst + zstep] - z0;
    zprev = z0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (r >= 4 && r < 12) continue;
      sp[r] = cmul(sp[r], tf_cis(z0, sq[r], false));
      dstep[rec_kslot(r)] = rec_step_factor(dz, sq[r], false);
      __builtin_amdgcn_sched_barrier(0);  // one double evaluation at a time, as in asm_cols_body
    }
  }
  for (int it = 0; it < nz; ++it) {
    const int zz = zfirst + it * zstep;
    const float z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(zl[zz])));
    const int M = mz[zz];
    const int Ms = __builtin_amdgcn_readfirstlane(M);
    float2 acc = make_float2(0.f, 0.f);
    if (rec) {
      if (it > 0) {
        const float eps = tf_sub(tf_sub(z, zprev), dz);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (r >= 4 && r < 12) continue;
          sp[r] = cmul(sp[r], dstep[rec_kslot(r)]);
        }
        // skipped on a scalar branch where the step is dz exactly (60 of cfg2's 63 steps)
        if (__builtin_amdgcn_readfirstlane(__float_as_int(eps)) != 0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (r >= 4 && r < 12) continue;
            sp[r] = rec_correct(sp[r], eps * sq[r]);
          }
        }
      }
      zprev = z;
      if (Ms != Mprev) {  // the band's edge: elements that leave the band are zeroed for good
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (r >= 4 && r < 12) continue;
          if (!rec_keep<PN>(r, tid, Ms)) sp[r] = make_float2(0.f, 0.f);
        }
      }
      Mprev = Ms;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r >= 4 && r < 12) continue;
        acc = cadd(acc, sp[r]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (sincos_keep<PN>(r, tid, M, Ms)) acc = cadd(acc, cmul(sp[r], tf_cis(z, sq[r], false)));
    }
    for (int o = 32; o > 0; o >>= 1) {
      acc.x += __shfl_xor(acc.x, o);
      acc.y += __shfl_xor(acc.y, o);
    }
    if (lane == 0) part[zz * nw + wave] = acc;
  }
  __syncthreads();
  for (int zz = tid; zz < nz; zz += nt) {
    float2 v = part[zz * nw];
    for (int w = 1; w < nw; ++w) v = cadd(v, part[zz * nw + w]);
    V[((size_t)(z_lo + zz) * a.BC + bc) * a.ncols + c] = v;
  }
}

// PN > 0: the compile-time power-of-two row transform of asm_rows_inv with a plain loader (V holds
// one value per band column); PN == 0: the runtime plan, data staged through LDS.
template <int PN>
__global__ void __launch_bounds__(1024) asm_rows_slice(const float2* __restrict__ V, float2* __restrict__ out,
                                                      FftPlan pw, AsmArgs a) {
  extern __shared__ float2 lds[];
  const int plane = blockIdx.x;  // zz * BC + bc
  const int tid = threadIdx.x, nt = blockDim.x;
  const float2* src = V + (size_t)plane * a.ncols;
  float2* dst = out + ((size_t)a.zoff * a.BC + plane) * a.Wout;
  if constexpr (PN > 0) {
    constexpr int TT = Geo<PN>::T;
    const auto twf = tw_fetch<PN, TT>(pw.tw, tid);
    const TwLds twl = tw_lds_at<PN>(tw_slot<PN>(lds));
    auto tw_hook = [&]() { tw_store<PN, TT>(tw_slot<PN>(lds), twf, tid); };
    auto ld = [&](int, int, int j) {
      const int c = band_col(j, PN, a.J, a.ncols);
      return c >= 0 ? src[c] : make_float2(0.f, 0.f);
    };
    auto sv = [&](int, int, int j, float2 v) {
      const int w = j - a.out_c0;
      if ((unsigned)w < (unsigned)a.Wout) dst[w] = v;
    };
    fft_pow2_run<true, PN, TT, FFT_ROWS>(lds, twl, tid, ld, sv, tw_hook);
  } else {
    for (int j = tid; j < a.Pw; j += nt) {
      const int c = band_col(j, a.Pw, a.J, a.ncols);
      lds[padx(j)] = c >= 0 ? src[c] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    fft_lds<true>(lds, pw, tid, nt);
    for (int w = tid; w < a.Wout; w += nt) dst[w] = lds[padx(a.out_c0 + w)];
  }
}

// ---------------------------------------------------------------------------------------------
// Adjoint of the z-x slice (thz_asm_slice_adjoint): g [Z][BC][Wo] -> gx [BC][H][W] = A_R^H g.
//   K1  rows_fwd      : the forward Pw-point transform of each cotangent row, band columns kept
//                       (asm_rows_fwd on a one-row geometry) -> Gv[z][bc][c]
//   K2a cols_slice_adj: per (bc, band column): Q[m] = conj(scale exp(2 pi i m R / Ph))
//                       sum_z conj(H_z(m)) Gv[z], one unnormalised inverse Ph-point transform,
//                       rows in_r0 .. in_r0 + H - 1 of it -> U (one plane)
//   K3  rows_inv      : asm_rows_inv on U -> gx
// `a` is the adjoint's argument block (in_* the forward's output window, out_* its input window).
// ---------------------------------------------------------------------------------------------
// One whole-column task per (bc, c); the planes are summed in segments of SLICE_ZC planes, each
// with the forward's own votes, plane order, anchor and step factors (asm_cols_slice's helpers,
// conjugated; the Horner loop and its registers are this kernel's own), so the recurrence never
// runs more than SLICE_ZC steps from a sincos anchor.  Under the recurrence H_j = A prod_{k <= j} s_k
// (A the anchor, s_k = D (1 + i eps_k sq)) and the segment's sum is a polynomial in the conjugate
// steps, run as Horner steps from the segment's far plane inward: acc = (acc + Gv_j) conj(s_j), and
// conj(A) once at the end.  The band
// only narrows in the order the planes are run, so an element enters the sum at the last plane
// that still holds it.  Every sum runs in a fixed order in registers: two calls are bit-identical.
template <int PN>
__global__ void __launch_bounds__(1024) asm_cols_slice_adj(const float2* __restrict__ Gv, float2* __restrict__ U,
                                                          FftPlan ph, AsmArgs a, int R) {
  extern __shared__ float2 lds[];
  using S = Pow2Sched<PN>;
  constexpr int TT = Geo<PN>::T;
  static_assert(S::radix(S::NST - 1, true) == 16 && PN / 16 / TT == 1, "one radix-16 butterfly per thread");
  static_assert(lds_floats2(PN) >= THZ_MAX_Z, "the column's Gv values fit the transform image");
  const int id = xcd_chunk(blockIdx.x, gridDim.x);
  const int bc = id / a.ncols, c = id - bc * a.ncols;
  const int nt = blockDim.x, Z = a.nz;
  const float lam = a.lam[bc % a.C];
  const float Ky = kfreq(c - a.J, a.Pw, a.dy);
  const int tid = threadIdx.x;
  const TwLds twl = load_tw_lds<PN>(lds + lds_floats2(PN), ph.tw, threadIdx.x, blockDim.x);
  // the column's Gv values in the transform image (free until the inverse transform): read
  // wave-uniform in the z loops
  float2* gl = lds;
  const auto [mz, zok, zl] = col_lds<PN>(lds);
  const float kl = TWO_PI_F / lam;
  const float kl2 = tf_mul(kl, kl);
  const float Ky2 = tf_mul(Ky, Ky);
  for (int zz = tid; zz < Z; zz += nt) {
    gl[zz] = Gv[((size_t)zz * a.BC + bc) * a.ncb * CB + c];
    const float zq = zval(a, zz);
    zl[zz] = zq;
    mz[zz] = tf_band_bound<PN>(a, a.Ph, tf_scalars(a, lam, zq), Ky);
    // the votes of the plane's own segment [s0, s0 + nzs), as asm_cols_slice takes them per launch
    const int s0 = zz / SLICE_ZC * SLICE_ZC, nzs = min(SLICE_ZC, Z - s0);
    zok[zz] = recurrence_votes([&](int k) { return zval(a, s0 + k); }, zz - s0, nzs, kl);
  }
  float sq[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) sq[r] = col_sq<PN>(tid + r * (PN / 16), a, kl2, Ky2);
  __syncthreads();  // gl, mz, zok, zl visible
  float2 qs[16];    // Q, element tid + r PN/16
#pragma unroll
  for (int r = 0; r < 16; ++r) qs[r] = make_float2(0.f, 0.f);
  for (int s0 = 0; s0 < Z; s0 += SLICE_ZC) {
    const int nzs = min(SLICE_ZC, Z - s0);
    bool rec, rev;
    recurrence_order<PN>(mz + s0, zok + s0, nzs, a.zrec, rec, rev);
    if (rec) {
      const int zfirst = rev ? s0 + nzs - 1 : s0, zstep = rev ? -1 : 1;
      const float z0 = zl[zfirst];
      const float dz = zl[zfirst + zstep] - z0;
      float2 acc[8], dstep[8];  // the kept values r < 4 (slots 0..3) and r >= 12 (4..7)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r >= 4 && r < 12) continue;
        dstep[rec_kslot(r)] = rec_step_factor(dz, sq[r], true);
        acc[rec_kslot(r)] = make_float2(0.f, 0.f);
        __builtin_amdgcn_sched_barrier(0);  // one double evaluation at a time, as in asm_cols_slice
      }
      for (int it = nzs - 1; it >= 0; --it) {
        const int zz = zfirst + it * zstep;
        const int Ms = __builtin_amdgcn_readfirstlane(mz[zz]);
        const float gx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gl[zz].x)));
        const float gy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gl[zz].y)));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (r >= 4 && r < 12) continue;
          const bool keep = rec_keep<PN>(r, tid, Ms);
          float2& v = acc[rec_kslot(r)];
          v.x += keep ? gx : 0.f;
          v.y += keep ? gy : 0.f;
        }
        if (it > 0) {
          const float z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(zl[zz])));
          const float zprev = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(zl[zz - zstep])));
          const float eps = tf_sub(tf_sub(z, zprev), dz);
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[k] = cmul(acc[k], dstep[k]);
          if (__builtin_amdgcn_readfirstlane(__float_as_int(eps)) != 0) {  // conj(1 + i eps sq)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              if (r >= 4 && r < 12) continue;
              acc[rec_kslot(r)] = rec_correct(acc[rec_kslot(r)], -(eps * sq[r]));
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r >= 4 && r < 12) continue;
        qs[r] = cadd(qs[r], cmul(acc[rec_kslot(r)], tf_cis(z0, sq[r], true)));
      }
    } else {
      for (int zz = s0; zz < s0 + nzs; ++zz) {
        const float z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(zl[zz])));
        const int M = mz[zz];
        const int Ms = __builtin_amdgcn_readfirstlane(M);
        const float gx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gl[zz].x)));
        const float gy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gl[zz].y)));
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (sincos_keep<PN>(r, tid, M, Ms)) qs[r] = cadd(qs[r], cmul(make_float2(gx, gy), tf_cis(z, sq[r], true)));
      }
    }
  }
  // Q[m] = conj(exp(2 pi i ((m R) mod Ph) / Ph) / (Ph Pw)) x the sum
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float2 p = slice_row_phase<PN>(tid, r, R);
    qs[r] = cmul(cscale(qs[r], a.scale), make_float2(p.x, -p.y));
  }
  __syncthreads();  // every wave is done with gl before the transform writes its image
  int tz = threadIdx.x;
  asm volatile("" : "+v"(tz));
  auto ld1 = [&](int, int r, int) { return qs[r]; };
  float2* dst = U + (size_t)bc * a.ncbu * CBU * u_rows(a.Hout) + blk_u(c, 0, a.Hout);
  auto sv1 = [&](int, int, int j, float2 v) {
    const int r = j - a.out_r0;
    if ((unsigned)r < (unsigned)a.Hout) dst[u_roff(r)] = v;
  };
  fft_pow2_io<true, PN, TT, FFT_TAIL, false, false>(lds, twl, tz, ld1, sv1);
}


// ---------------------------------------------------------------------------------------------
// RSC (Props/RSC_Prop.py:129-215): transfer function = FFT2 of the spatial RS kernel on the
// P = N + 2 floor(N/2) grid, stored column-major [C][Pw][Ph] for the column pass.
// ---------------------------------------------------------------------------------------------
struct RscKArgs {
  int C, Ph, Pw, ncbK;
  float dx, z;
  float lam[THZ_MAX_WAVELENGTHS];
};

template <int PN>
__global__ void __launch_bounds__(1024) rsc_k_rows(float2* __restrict__ TK, FftPlan pw, RscKArgs k) {
  extern __shared__ float2 lds[];
  const int row = blockIdx.x;
  const int c = row / k.Ph, i = row - c * k.Ph;
  const float lam = k.lam[c];
  const float kk = 6.283185307179586f / lam;
  const RsPhase rph = rs_phase(lam, k.z);
  // grid x = linspace(-P dx/2, P dx/2, P) on both axes with dx (:83-84)
  const float xi = lin(-(float)k.Ph * k.dx / 2.0f, (float)k.Ph * k.dx / 2.0f, k.Ph, i);
  const float ylo = -(float)k.Pw * k.dx / 2.0f, yhi = (float)k.Pw * k.dx / 2.0f;
  float2* dst = TK + (size_t)c * k.ncbK * CB * k.Ph;
  auto load = [&](int j) { return rs_kernel(xi, lin(ylo, yhi, k.Pw, j), k.z, kk, rph); };
  auto store = [&](int j, float2 v) { dst[blk(band_col(j, k.Pw, k.Pw / 2, k.Pw), i, k.Ph)] = v; };
  const int tid = threadIdx.x, nt = blockDim.x;
  if constexpr (PN > 0) {
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), pw.tw, tid, nt);
    auto ld = [&](int, int, int j) { return load(j); };
    auto sv = [&](int, int, int j, float2 v) { store(j, v); };
    fft_pow2_run<false, PN, Geo<PN>::T, FFT_ROWS>(lds, twl, tid, ld, sv);
  } else {
    for (int j = tid; j < k.Pw; j += nt) lds[padx(j)] = load(j);
    __syncthreads();
    fft_lds<false>(lds, pw, tid, nt);
    for (int j = tid; j < k.Pw; j += nt) store(j, lds[padx(j)]);
  }
}

template <int PN>
__global__ void __launch_bounds__(1024) rsc_k_cols(const float2* __restrict__ TK, float2* __restrict__ KF,
                                                  FftPlan ph, RscKArgs k) {
  extern __shared__ float2 lds[];
  const int id = xcd_chunk(blockIdx.x, gridDim.x);
  const int c = id / k.Pw, cc = id - c * k.Pw;
  const float2* col = TK + (size_t)c * k.ncbK * CB * k.Ph + blk(cc, 0, k.Ph);
  float2* dst = KF + ((size_t)c * k.Pw + cc) * k.Ph;
  const int tid = threadIdx.x, nt = blockDim.x;
  if constexpr (PN > 0) {
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), ph.tw, tid, nt);
    auto ld = [&](int, int, int i) { return col[(size_t)i * CB]; };
    auto sv = [&](int, int, int i, float2 v) { dst[i] = v; };
    fft_pow2_run<false, PN, Geo<PN>::T, FFT_ROWS>(lds, twl, tid, ld, sv);
  } else {
    for (int i = tid; i < k.Ph; i += nt) lds[padx(i)] = col[(size_t)i * CB];
    __syncthreads();
    fft_lds<false>(lds, ph, tid, nt);
    for (int i = tid; i < k.Ph; i += nt) dst[i] = lds[padx(i)];
  }
}

// ---------------------------------------------------------------------------------------------
// Generic batched row FFT (building block / diagnostics)
// ---------------------------------------------------------------------------------------------
template <int PN>
__global__ void __launch_bounds__(1024) fft_rows_kernel(const float2* __restrict__ in, float2* __restrict__ out,
                                                       FftPlan p, int inverse, size_t stride) {
  extern __shared__ float2 lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const size_t base = (size_t)blockIdx.x * stride;
  if constexpr (PN > 0) {
    const TwLds twl = load_tw_lds<PN>(tw_slot<PN>(lds), p.tw, tid, nt);
    auto ld = [&](int, int, int j) { return in[base + j]; };
    auto sv = [&](int, int, int j, float2 v) { out[base + j] = v; };
    if (inverse) fft_pow2_run<true, PN, Geo<PN>::T, 3>(lds, twl, tid, ld, sv);
    else fft_pow2_run<false, PN, Geo<PN>::T, FFT_TAIL>(lds, twl, tid, ld, sv);
  } else {
    for (int j = tid; j < p.n; j += nt) lds[padx(j)] = in[base + j];
    __syncthreads();
    if (inverse) fft_lds<true>(lds, p, tid, nt);
    else fft_lds<false>(lds, p, tid, nt);
    for (int j = tid; j < p.n; j += nt) out[base + j] = lds[padx(j)];
  }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
struct AsmGeom {
  int BC, Ph, Pw, ncols, J, ncb, ncbu, Hin, Win, Hout, Wout, zc;
  int C;
  int adj;  // adjoint: T holds the z-chunk's planes, U one (summed) plane
};

static int validate(const thz_asm_desc* d) {
  if (!d) return fail(THZ_E_ARG, "null descriptor");
  if (d->B < 1 || d->C < 1 || d->H < 1 || d->W < 1 || d->pad_h < 0 || d->pad_w < 0)
    return fail(THZ_E_ARG, "bad shape B=%d C=%d H=%d W=%d pad=(%d,%d)", d->B, d->C, d->H, d->W, d->pad_h, d->pad_w);
  if (d->C > THZ_MAX_WAVELENGTHS) return fail(THZ_E_UNSUPPORTED, "C=%d > %d wavelengths", d->C, THZ_MAX_WAVELENGTHS);
  if (d->Z < 1 || d->Z > THZ_MAX_Z) return fail(THZ_E_UNSUPPORTED, "Z=%d outside [1, %d]", d->Z, THZ_MAX_Z);
  if (d->bandlimit < 0 || d->bandlimit > 2) return fail(THZ_E_ARG, "bad bandlimit %d", d->bandlimit);
  if (!d->wavelengths || (!d->z && !d->z_dev)) return fail(THZ_E_ARG, "null wavelengths / z");
  if (!(d->dx > 0.f) || !(d->dy > 0.f)) return fail(THZ_E_ARG, "spacing must be > 0");
  const int Ph = d->H + 2 * d->pad_h, Pw = d->W + 2 * d->pad_w;
  if (Ph > FFT_MAX_N || Pw > FFT_MAX_N)
    return fail(THZ_E_UNSUPPORTED, "padded size %dx%d exceeds %d", Ph, Pw, FFT_MAX_N);
  for (int c = 0; c < d->C; ++c)
    if (!(d->wavelengths[c] > 0.f)) return fail(THZ_E_ARG, "wavelength[%d] must be > 0", c);
  return THZ_OK;
}

// Largest |m_y| with a possibly non-zero H over all (wavelength, z); +2 columns margin for
// the fp32-vs-double evaluation.  Exact: Ky^2 <= min(k^2, (2 pi v_lim)^2); approx: |Ky| <=
// min(k, k_y_max); none: evanescent only.  All maxima sit on the Kx = 0 row.
static int band_half_width(const thz_asm_desc* d, int Ph, int Pw) {
  double kymax = 0.0;
  const double dy = d->dy, dx = d->dx;
  for (int c = 0; c < d->C; ++c) {
    const double lam = d->wavelengths[c];
    const double kl = 2.0 * M_PI / lam;
    for (int zi = 0; zi < d->Z; ++zi) {
      double lim = kl;
      if (d->z_dev) {  // the planes are read on the device: size the band for any z (evanescent bound)
        kymax = std::max(kymax, lim);
        continue;
      }
      const double z = d->z[zi];
      if (d->bandlimit == THZ_BANDLIMIT_EXACT) {
        const double dv = 1.0 / (2.0 * Ph * dy);
        const double vl = 1.0 / std::sqrt(std::pow(2.0 * dv * z, 2) + 1.0) / lam;
        lim = std::min(lim, 2.0 * M_PI * vl);
      } else if (d->bandlimit == THZ_BANDLIMIT_APPROX) {
        const double ly = Ph * dy;
        const double kym = 2.0 * M_PI / std::sqrt(std::pow(2.0 * z / ly, 2) + 1.0) / lam;
        lim = std::min(lim, kym);
      }
      kymax = std::max(kymax, lim);
    }
  }
  (void)dx;
  const double dky = 2.0 * M_PI / (Pw * dy);
  const double j = std::floor(kymax / dky) + 2.0;
  if (j >= Pw / 2) return -1;  // full band
  return (int)j;
}

static void geometry(const thz_asm_desc* d, AsmGeom* g) {
  g->BC = d->B * d->C;
  g->C = d->C;
  g->Ph = d->H + 2 * d->pad_h;
  g->Pw = d->W + 2 * d->pad_w;
  const int Ho = d->unpad ? d->H : g->Ph, Wo = d->unpad ? d->W : g->Pw;
  if (!d->adjoint) {
    g->Hin = d->H; g->Win = d->W; g->Hout = Ho; g->Wout = Wo;
  } else {
    g->Hin = Ho; g->Win = Wo; g->Hout = d->H; g->Wout = d->W;
  }
  const int J = band_half_width(d, g->Ph, g->Pw);
  if (J < 0) {
    g->ncols = g->Pw;
    g->J = g->Pw / 2;
  } else {
    g->ncols = 2 * J + 1;
    g->J = J;
  }
  g->ncb = (g->ncols + CB - 1) / CB;
  g->ncbu = (g->ncols + CBU - 1) / CBU;
  int zc = d->z_chunk > 0 ? d->z_chunk : 0;
  if (zc == 0) {
    // default: up to 64 z-planes per column pass (the forward column FFT and the T read are
    // shared by the chunk; one K2 and one K3 launch per 64 planes), U capped at 10 GiB of the
    // 288 GB HBM.  Measured on cfg2 (64 planes, round 2): z_chunk 32 / 64 -> 6830 / 7270 planes/s.
    // The Z-summing adjoint keeps the chunk's input planes in T instead (same cap).
    const double per_z = d->adjoint ? (double)g->BC * g->ncb * CB * g->Hin * sizeof(float2)
                                    : (double)g->BC * g->ncbu * CBU * u_rows(g->Hout) * sizeof(float2);
    zc = (int)std::max(1.0, std::min(64.0, std::floor((10240.0 * 1024 * 1024) / per_z)));
  }
  g->zc = std::min(zc, d->Z);
  g->adj = d->adjoint;
}

// The argument block every pipeline on this file starts from: the sizes and window sizes of the
// geometry, the band, the spacings, the transform's 1 / (Ph Pw) and the wavelengths.  The callers
// add what is theirs: the windows' origins, the direction and the planes.
static AsmArgs args_base(const AsmGeom& g, int bandlimit, float dx, float dy, const float* wavelengths) {
  AsmArgs a{};
  a.BC = g.BC;
  a.C = g.C;
  a.Ph = g.Ph;
  a.Pw = g.Pw;
  a.Hin = g.Hin; a.Win = g.Win; a.Hout = g.Hout; a.Wout = g.Wout;  // geometry(): the windows' sizes
  a.ncols = g.ncols;
  a.ncb = g.ncb;
  a.ncbu = g.ncbu;
  a.J = g.J;
  a.bl = bandlimit;
  a.dx = dx;
  a.dy = dy;
  a.scale = (float)(1.0 / ((double)g.Ph * (double)g.Pw));
  for (int c = 0; c < g.C; ++c) a.lam[c] = wavelengths[c];
  return a;
}

// The argument block as every ASM entry point starts it: the base, the forward's windows or
// (d->adjoint) the adjoint's, and the planes.
static AsmArgs asm_args_base(const thz_asm_desc* d, const AsmGeom& g) {
  AsmArgs a = args_base(g, d->bandlimit, d->dx, d->dy, d->wavelengths);
  const int o_r0 = d->unpad ? d->pad_h : 0, o_c0 = d->unpad ? d->pad_w : 0;
  a.in_r0 = d->adjoint ? o_r0 : d->pad_h; a.in_c0 = d->adjoint ? o_c0 : d->pad_w;
  a.out_r0 = d->adjoint ? d->pad_h : o_r0; a.out_c0 = d->adjoint ? d->pad_w : o_c0;
  a.adjoint = d->adjoint;
  if (d->z)
    for (int zi = 0; zi < d->Z; ++zi) a.zv[zi] = d->z[zi];
  a.zdev = d->z_dev;
  return a;
}

// ---- the mixed-radix dispatchers (the size list and its dispatchers: thz_launch.hpp) -----------
// the row passes K1 / K3: the mixed-radix instantiations, then as on_pow2
template <class F>
static void on_rows(int n, F&& f) {
  if (!on_listed(SizeList<Mx300::N, Mx500::N>{}, n, f)) on_pow2(n, f);
}
// the mixed-radix column pass and its tables, templated on the plan: f(Mx300{}) or f(Mx500{})
template <class F>
static void on_mx(int n, F&& f) {
  if (n == Mx300::N) f(Mx300{});
  else f(Mx500{});
}
// workgroup size of the row passes (the mixed-radix instantiations before threads_for's)
static int rows_threads(int n) { return is_mx(n) ? mx_threads(n) : threads_for(n); }

// Dynamic LDS of the column passes, one definition per kernel family.  Power of two and runtime
// plan: the transform, then mz, zok and the z values (ColLds); their Z-summing form keeps mz only;
// the mixed-radix kernels hold the data rows (their twiddles live in registers) and mz.
static size_t k2_lds_bytes(int Ph) { return fft_lds_bytes(Ph) + 12 * THZ_MAX_Z; }
static size_t k2_zsum_lds_bytes(int Ph) { return fft_lds_bytes(Ph) + 4 * THZ_MAX_Z; }
static size_t k2_mx_lds_bytes(int Ph) { return lds_floats2(Ph) * sizeof(float2) + 4 * THZ_MAX_Z; }

// The large-LDS opt-in (lds_opt_in) of this unit, once: every kernel of the power-of-two and
// runtime-plan sizes (the mixed-radix ones stay far below 64 KiB).
static int ensure_lds_attr() {
  static const int rc = [] {
    std::vector<const void*> ks;
    auto planes = [&](auto N) {
      constexpr int PN = N();
      ks.insert(ks.end(), {(const void*)asm_rows_fwd<PN>, (const void*)asm_cols<PN>, (const void*)asm_cols_zsum<PN>,
                           (const void*)asm_rows_inv<PN>, (const void*)asm_rows_inv_loss<PN>,
                           (const void*)asm_rows_slice<PN>, (const void*)fft_rows_kernel<PN>,
                           (const void*)rsc_k_rows<PN>, (const void*)rsc_k_cols<PN>});
      if constexpr (PN == 8192)
        ks.insert(ks.end(), {(const void*)asm_rows_inv_mid<PN>, (const void*)asm_rows_inv_pair<PN, true>});
      if constexpr (PN > 0)  // the families of the compile-time sizes only
        ks.insert(ks.end(), {(const void*)asm_rows_inv_pair<PN, false>, (const void*)asm_cols_slice<PN>,
                             (const void*)asm_cols_slice_adj<PN>});
    };
    for_each_size(Pow2Sizes{}, planes);
    planes(Size<0>{});
    return lds_opt_in(ks, k2_lds_bytes(FFT_MAX_N));
  }();
  return rc;
}

// The 300-point passes with the layers' windows ([N/3, 2N/3) in and out: padding 2 with unpad,
// cfg4 / cfg5) as compile-time constants: the column pass (asm_cols_mx_mid: 80.8 vs 83.3 us per
// launch, cfg5 chained 1.097 vs 1.133 ms), K1 (asm_rows_fwd<300, true>) and K3
// (asm_rows_inv_mid<300>, asm_rows_inv_loss_mid<300>).  The A/B records: profiles/r04_experiments.txt.
static bool mx_mid(int Ph, const AsmArgs& a) {
  return Ph == Mx300::N && !a.tft && a.in_r0 == Mx300::N / 3 && a.Hin == Mx300::N / 3 && a.out_r0 == Mx300::N / 3 &&
         a.Hout == Mx300::N / 3;
}
// K3 with its crop as a compile-time window: the middle half of P = 8192 (asm_rows_inv_mid<8192>,
// padding scale 1 with unpad, cfg2: 4.00 vs 4.13 ms) or the middle third of P = 300
static bool k3_mid(int Pw, const AsmArgs& a) {
  return (Pw == 8192 && a.out_c0 == Pw / 4 && a.Wout == Pw / 2) ||
         (Pw == Mx300::N && a.out_c0 == Pw / 3 && a.Wout == Pw / 3);
}
// K1 of the 300-point layers with the input window as constants (asm_rows_fwd<300, true>)
static bool k1_mid(int Pw, const AsmArgs& a) { return Pw == Mx300::N && a.in_c0 == Pw / 3 && a.Win == Pw / 3; }

// every row and column pass of the planes' pipelines has this signature
using PassKernel = void (*)(const float2*, float2*, FftPlan, AsmArgs);

// the column pass of the planes (asm_cols, or asm_cols_mx on a mixed-radix height)
static PassKernel cols_kernel(int Ph) {
  PassKernel k = nullptr;
  if (is_mx(Ph)) on_mx(Ph, [&](auto P) { k = asm_cols_mx<decltype(P)>; });
  else on_pow2(Ph, [&](auto N) { k = asm_cols<N()>; });
  return k;
}

// Workgroups of the column pass resident on the whole device at once (CUs x occupancy).
static int k2_resident(int Ph, int threads, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int, size_t>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lk(mu);
  auto key = std::make_tuple(dev, Ph, threads, lds);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)cols_kernel(Ph), threads, lds) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    per_cu = cus = 0;
  const int r = per_cu * cus;
  cache[key] = r;
  return r;
}

// K2 task split: whole columns for the full dispatch rounds, the remainder split by z-range.
static int k2_tasks(const AsmGeom& g, AsmArgs* a, int threads, size_t lds) {
  const int nc = g.ncols * g.BC;
  const int G = k2_resident(g.Ph, threads, lds);
  if (G <= 0 || a->nz <= 1) {
    a->kfull = nc;
    a->kparts = 1;
    return nc;
  }
  const int full = nc / G * G, rem = nc - full;
  a->kfull = full;
  a->kparts = rem ? std::max(1, std::min(a->nz, G / rem)) : 1;
  return full + rem * a->kparts;
}

// THZ_K2_RECURRENCE=0 keeps the per-plane sincos everywhere (the A/B and parity tests compare the
// two forms; read per call so a test can toggle it)
static bool plane_recurrence_disabled() {
  const char* v = std::getenv("THZ_K2_RECURRENCE");
  return v && v[0] == '0';
}

// ---- workspace layouts -----------------------------------------------------------------------
// T: K1's band spectra, one plane (the Z-summing adjoint: the z-chunk's planes)
static size_t t_bytes(const AsmGeom& g) {
  return align256((size_t)(g.adj ? g.zc : 1) * g.BC * g.ncb * CB * g.Hin * sizeof(float2));
}
// U: `planes` planes of column-pass output in the layout K3 gathers
static size_t u_bytes(const AsmGeom& g, int planes) {
  return align256((size_t)planes * g.BC * g.ncbu * CBU * u_rows(g.Hout) * sizeof(float2));
}
// the mixed-radix column pass's per-(wavelength, column) tables, shared by every plane: sqt, then mzt
static size_t tab_sq_bytes(const AsmGeom& g) { return align256((size_t)g.C * g.ncols * g.Ph * sizeof(float)); }
static size_t tab_bytes(const AsmGeom& g) {
  return is_mx(g.Ph) ? tab_sq_bytes(g) + align256((size_t)g.C * g.ncols * g.zc * sizeof(int)) : 0;
}
// planes per cols_slice launch: the full path's z-chunk (so the recurrence starts where it does
// there), at most SLICE_ZC
static int slice_zc(const AsmGeom& g) { return std::min(g.zc, SLICE_ZC); }

// Which pipeline an entry point runs: it decides the validation and the workspace layout.
enum class Pipe { Planes, Slice, SliceAdjoint };

// A pipeline's workspace, part by part in address order.  The *_workspace_size entries return the
// sum and asm_plan() cuts the caller's workspace by the same parts.
struct WsLayout {
  size_t part[3];
  size_t total() const { return part[0] + part[1] + part[2]; }
};
static WsLayout ws_layout(Pipe pipe, const AsmGeom& g, int Z) {
  switch (pipe) {
    case Pipe::Slice:  // T | V [zc][BC][ncols]
      return {{t_bytes(g), align256((size_t)slice_zc(g) * g.BC * g.ncols * sizeof(float2)), 0}};
    case Pipe::SliceAdjoint:  // (g: the adjoint descriptor's, Hout x Wout the field) U of one plane | Gv [Z][BC][ncb CB]
      return {{u_bytes(g, 1), align256((size_t)Z * g.BC * g.ncb * CB * sizeof(float2)), 0}};
    default:  // T | U of a z-chunk (the Z-summing adjoint: one plane) | the mixed-radix tables
      return {{t_bytes(g), u_bytes(g, g.adj ? 1 : g.zc), tab_bytes(g)}};
  }
}

// what a call needs of the device before its first launch: the FFT plans of both axes and the
// kernels' large-LDS opt-in
static int device_plans(const AsmGeom& g, FftPlan* pw, FftPlan* ph) {
  int e;
  if ((e = get_plan(g.Pw, pw)) || (e = get_plan(g.Ph, ph))) return e;
  return ensure_lds_attr();
}

// ---- the launch plan -------------------------------------------------------------------------
// One call's launch plan: what the stage launchers need besides the z-chunk's argument block.
struct AsmPlan {
  AsmGeom g;
  FftPlan pw, ph;
  AsmArgs a;     // as the entry prepared it; the run_* loops work on a copy
  hipStream_t s;
  int Z;
  char* ws[3];   // the workspace parts of ws_layout (nullptr: an empty part)
};

// K1 over `planes` input planes of a.Hin rows.  a.tab_blocks further workgroups compute the first
// z-chunk's column tables (run_pipeline).
static int launch_k1(const AsmPlan& p, const AsmArgs& a, int planes, const void* in, float2* T) {
  const int Pw = p.g.Pw;
  PassKernel k = nullptr;
  if (k1_mid(Pw, a)) k = asm_rows_fwd<Mx300::N, true>;
  else on_rows(Pw, [&](auto N) { k = asm_rows_fwd<N()>; });
  KernelTimer kt("asm_rows_fwd", p.s);
  hipLaunchKernelGGL(k, dim3(planes * a.BC * a.Hin + a.tab_blocks), dim3(rows_threads(Pw)), fft_lds_bytes_io(Pw), p.s,
                     (const float2*)in, T, p.pw, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

// The column pass of the z-chunk [a.zoff, a.zoff + a.nz): the planes' (split into k2_tasks) or, with
// a.zsum, the Z-summing adjoint's (every column task runs all of its chunk's planes).  `tables`: the
// mixed-radix tables of this chunk first, inside the same timer bracket.
static int launch_cols(const AsmPlan& p, AsmArgs& a, bool tables, const float2* T, float2* U) {
  const AsmGeom& g = p.g;
  const bool mx = is_mx(g.Ph);
  const int th = mx ? mx_threads(g.Ph) : threads_for(g.Ph);
  const size_t lds = mx ? k2_mx_lds_bytes(g.Ph) : a.zsum ? k2_zsum_lds_bytes(g.Ph) : k2_lds_bytes(g.Ph);
  PassKernel k = nullptr;
  if (a.zsum) {
    if (mx) on_mx(g.Ph, [&](auto P) { k = asm_cols_mx_zsum<decltype(P)>; });
    else on_pow2(g.Ph, [&](auto N) { k = asm_cols_zsum<N()>; });
  } else {
    k = mx_mid(g.Ph, a) ? asm_cols_mx_mid<Mx300> : cols_kernel(g.Ph);
  }
  KernelTimer kt("asm_cols", p.s);
  if (tables) {
    on_mx(g.Ph, [&](auto P) {
      hipLaunchKernelGGL(asm_tf_tables<decltype(P)::N>, dim3(g.C * g.ncols), dim3(MX_T), 0, p.s, a, a.zoff == 0);
    });
    THZ_LAUNCH_CHECK();
  }
  int ntask = g.ncols * g.BC;
  if (a.zsum) {
    a.kfull = ntask;
    a.kparts = 1;
  } else {
    ntask = k2_tasks(g, &a, th, lds);
    if (!mx) a.zrec = !plane_recurrence_disabled();
  }
  hipLaunchKernelGGL(k, dim3(ntask), dim3(th), lds, p.s, T, U, p.ph, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

// thz_asm_row_pairs: -1 the library's choice, 0 one row per workgroup, 1 row pairs wherever the
// pair kernel exists (read per call, so a parity test can run both forms in one process)
static std::atomic<int> g_row_pairs{-1};

// K3 on row pairs?  By default where it was measured: the middle-half crop of P = 8192 (cfg2, K3 per
// 64 planes: DESIGN.md §22); every plain power-of-two size when forced.
static bool k3_pairs(int Pw, bool loss, bool mid) {
  if (loss || !pow2_kind(Pw)) return false;
  const int mode = g_row_pairs.load(std::memory_order_relaxed);
  return mode < 0 ? mid && Pw == 8192 : mode > 0;
}

// K3 over the a.nz planes in U: plain, or with the loss sums (a.ls), each also with the crop as
// constants (k3_mid); the plain power-of-two form also on row pairs (k3_pairs)
static int launch_k3(const AsmPlan& p, const AsmArgs& a, const float2* U, void* out) {
  const int Pw = p.g.Pw;
  const bool loss = a.ls.stats != nullptr, mid = k3_mid(Pw, a), pairs = k3_pairs(Pw, loss, mid);
  PassKernel k = nullptr;
  if (mid && Pw == Mx300::N) k = loss ? asm_rows_inv_loss_mid<Mx300::N> : asm_rows_inv_mid<Mx300::N>;
  else if (pairs && mid) k = asm_rows_inv_pair<8192, true>;
  else if (pairs) on_pow2_only(Pw, [&](auto N) { k = asm_rows_inv_pair<N(), false>; });
  else if (mid && !loss) k = asm_rows_inv_mid<8192>;
  else if (loss) on_rows(Pw, [&](auto N) { k = asm_rows_inv_loss<N()>; });
  else on_rows(Pw, [&](auto N) { k = asm_rows_inv<N()>; });
  KernelTimer kt("asm_rows_inv", p.s);
  const int rows = pairs ? (a.Hout + 1) / 2 : a.Hout;  // workgroups per plane
  hipLaunchKernelGGL(k, dim3(a.nz * a.BC * rows), dim3(rows_threads(Pw)), fft_lds_bytes_io(Pw, pairs ? 2 : 1), p.s, U,
                     (float2*)out, p.pw, a);
  THZ_LAUNCH_CHECK();
  int e;
  if (loss && (e = launch_loss_finish(a.ls, p.s))) return e;
  kt.stop();
  return THZ_OK;
}

// The z-x slice's column pass of the z-chunk, row R of the padded plane: T -> V (asm_cols' own task
// split), or its Z-summing adjoint Gv -> U (one task per column).
static int launch_cols_slice(const AsmPlan& p, AsmArgs& a, bool adjoint, const float2* src, float2* dst, int R) {
  const AsmGeom& g = p.g;
  const int th = threads_for(g.Ph);
  const size_t lds = k2_lds_bytes(g.Ph);
  void (*k)(const float2*, float2*, FftPlan, AsmArgs, int) = nullptr;
  const bool served = on_pow2_only(g.Ph, [&](auto N) {
    if (adjoint) k = asm_cols_slice_adj<N()>;
    else k = asm_cols_slice<N()>;
  });
  if (!served) return fail(THZ_E_UNSUPPORTED, "z-x slice: no column pass for padded height %d", g.Ph);
  a.zrec = !plane_recurrence_disabled();
  KernelTimer kt(adjoint ? "asm_cols_slice_adj" : "asm_cols_slice", p.s);
  const int ntask = adjoint ? g.ncols * g.BC : k2_tasks(g, &a, th, lds);
  hipLaunchKernelGGL(k, dim3(ntask), dim3(th), lds, p.s, src, dst, p.ph, a, R);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

// the z-x slice's row pass: one row per (plane of the chunk, bc), V -> out
static int launch_rows_slice(const AsmPlan& p, const AsmArgs& a, const float2* V, void* out) {
  const int Pw = p.g.Pw;
  PassKernel k = nullptr;
  on_pow2(Pw, [&](auto N) { k = asm_rows_slice<N()>; });
  KernelTimer kt("asm_rows_slice", p.s);
  hipLaunchKernelGGL(k, dim3(a.nz * a.BC), dim3(threads_for(Pw)), fft_lds_bytes_io(Pw), p.s, V, (float2*)out, p.pw, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

// ---- the z-chunk loops -----------------------------------------------------------------------
// The adjoint of a Z-plane forward (sum over planes): per z-chunk, K1 over the chunk's input
// planes and the Z-summing K2; then K3 once on the summed plane.
static int run_adjoint_sum(const AsmPlan& p, AsmArgs a, const void* in, void* out) {
  float2 *T = (float2*)p.ws[0], *U = (float2*)p.ws[1];
  int e;
  a.zsum = 1;
  a.tab_blocks = 0;  // K1 runs per chunk here: every chunk launches its tables itself
  for (int z0 = 0; z0 < p.Z; z0 += p.g.zc) {
    a.zoff = z0;
    a.nz = std::min(p.g.zc, p.Z - z0);
    a.zacc = z0 > 0;  // the chunks after the first add into U
    if ((e = launch_k1(p, a, a.nz, in, T))) return e;
    if ((e = launch_cols(p, a, a.sqt != nullptr, T, U))) return e;
  }
  a.zoff = 0;
  a.nz = 1;
  return launch_k3(p, a, U, out);
}

// K1 once, then (K2, K3) per z-chunk.  a.sqt is set where the column pass takes its tables from the
// workspace (asm_forward_impl: the mixed-radix heights; the RSC pipeline brings a.tft instead).
static int run_pipeline(const AsmPlan& p, const void* in, void* out) {
  const AsmGeom& g = p.g;
  float2 *T = (float2*)p.ws[0], *U = (float2*)p.ws[1];
  AsmArgs a = p.a;
  if (g.adj && p.Z > 1) return run_adjoint_sum(p, a, in, out);
  int e;
  const bool tables = a.sqt != nullptr;
  // square 300-point grids (cfg4 / cfg5): the first z-chunk's column tables ride along with K1
  // (tf_tables_body<PN> of K1's own size: Ph == Pw), one launch fewer per layer
  a.tab_blocks = tables && g.Pw == g.Ph && g.Pw == Mx300::N ? g.C * g.ncols : 0;
  a.zoff = 0;
  a.nz = std::min(g.zc, p.Z);
  if ((e = launch_k1(p, a, 1, in, T))) return e;
  for (int z0 = 0; z0 < p.Z; z0 += g.zc) {
    a.zoff = z0;
    a.nz = std::min(g.zc, p.Z - z0);
    if ((e = launch_cols(p, a, tables && !(z0 == 0 && a.tab_blocks), T, U))) return e;
    if ((e = launch_k3(p, a, U, out))) return e;
  }
  return THZ_OK;
}

// K1 once, then (cols_slice, rows_slice) per z-chunk: row R of the padded plane
static int run_slice(const AsmPlan& p, int R, const void* in, void* out) {
  float2 *T = (float2*)p.ws[0], *V = (float2*)p.ws[1];
  AsmArgs a = p.a;
  int e;
  const int zc = slice_zc(p.g);
  a.zoff = 0;
  a.nz = std::min(zc, p.Z);
  if ((e = launch_k1(p, a, 1, in, T))) return e;
  for (int z0 = 0; z0 < p.Z; z0 += zc) {
    a.zoff = z0;
    a.nz = std::min(zc, p.Z - z0);
    if ((e = launch_cols_slice(p, a, false, T, V, R))) return e;
    if ((e = launch_rows_slice(p, a, V, out))) return e;
  }
  return THZ_OK;
}

// row pass over the Z BC cotangent rows, the Z-summing column pass, K3 once: no loop, the column
// pass segments the planes itself
static int run_slice_adjoint(const AsmPlan& p, int R, const void* gout, void* gin) {
  float2 *U = (float2*)p.ws[0], *Gv = (float2*)p.ws[1];
  AsmArgs a = p.a;
  int e;
  a.zoff = 0;
  a.nz = p.Z;
  // each cotangent row is a one-row plane: Gv[z][bc] is T of plane z BC + bc with Hin = 1
  AsmArgs a1 = a;
  a1.Hin = 1;
  a1.in_r0 = 0;
  if ((e = launch_k1(p, a1, p.Z, gout, Gv))) return e;
  if ((e = launch_cols_slice(p, a, true, Gv, U, R))) return e;
  a.nz = 1;
  return launch_k3(p, a, U, gin);
}

// what thz_asm_slice_* accept, checked on the host before any device call
static int validate_slice(const thz_asm_desc* d, bool adjoint) {
  int e = validate(d);
  if (e) return e;
  if (adjoint && d->adjoint != 1) return fail(THZ_E_ARG, "the z-x slice adjoint takes adjoint == 1");
  if (!adjoint && d->adjoint)
    return fail(THZ_E_UNSUPPORTED, "z-x slice: forward only (the adjoint is thz_asm_slice_adjoint)");
  if (d->z_dev) return fail(THZ_E_UNSUPPORTED, "z-x slice: host plane distances only (z_dev is not read)");
  if (!d->z) return fail(THZ_E_ARG, "null z");
  if (d->window_mask) return fail(THZ_E_UNSUPPORTED, "z-x slice: no window mask (apply the aperture separately)");
  const int Ph = d->H + 2 * d->pad_h;
  if (!pow2_kind(Ph))
    return fail(THZ_E_UNSUPPORTED, "z-x slice: padded height %d is not one of 1024, 2048, 4096, 8192, 16384 "
                                   "(slice thz_asm_forward's planes instead)", Ph);
  return THZ_OK;
}
static int validate_pipe(const thz_asm_desc* d, Pipe pipe) {
  return pipe == Pipe::Planes ? validate(d) : validate_slice(d, pipe == Pipe::SliceAdjoint);
}

// The prelude of every entry that launches: the descriptor's validation, the geometry, the slices'
// row (of the forward's output grid), the data pointers (data_ok), the workspace against the
// pipeline's layout, the device plans and the argument block -- all host checks before any device call.
static int asm_plan(const thz_asm_desc* d, Pipe pipe, int row, bool data_ok, void* workspace, size_t bytes,
                    thz_stream_t stream, AsmPlan* p) {
  int e = validate_pipe(d, pipe);
  if (e) return e;
  AsmGeom& g = p->g;
  geometry(d, &g);
  if (pipe != Pipe::Planes) {
    // adjoint descriptor: Hin x Win is the forward's output grid, Hout x Wout the field
    const int rows = pipe == Pipe::Slice ? g.Hout : g.Hin;
    if (row < 0 || row >= rows)
      return fail(THZ_E_ARG, "z-x slice%s: row %d outside [0, %d)", pipe == Pipe::Slice ? "" : " adjoint", row, rows);
  }
  if (!data_ok) return fail(THZ_E_ARG, "null data pointer");
  const WsLayout lay = ws_layout(pipe, g, d->Z);
  if ((e = check_workspace(workspace, bytes, lay.total()))) return e;
  if ((e = device_plans(g, &p->pw, &p->ph))) return e;
  char* w = (char*)workspace;
  for (int i = 0; i < 3; ++i) {
    p->ws[i] = lay.part[i] ? w : nullptr;
    w += lay.part[i];
  }
  p->a = asm_args_base(d, g);
  p->s = (hipStream_t)stream;
  p->Z = d->Z;
  return THZ_OK;
}

static int asm_workspace_size(const thz_asm_desc* d, Pipe pipe, size_t* bytes) {
  int e = validate_pipe(d, pipe);
  if (e) return e;
  if (!bytes) return fail(THZ_E_ARG, "null bytes");
  AsmGeom g;
  geometry(d, &g);
  *bytes = ws_layout(pipe, g, d->Z).total();
  return THZ_OK;
}

}  // namespace thz

using namespace thz;

extern "C" int thz_asm_slice_workspace_size(const thz_asm_desc* d, size_t* bytes) {
  return asm_workspace_size(d, Pipe::Slice, bytes);
}

extern "C" int thz_asm_slice_forward(const thz_asm_desc* d, int row, const void* in, void* out, void* workspace,
                                     size_t workspace_bytes, thz_stream_t stream) {
  AsmPlan p;
  int e = asm_plan(d, Pipe::Slice, row, in && out, workspace, workspace_bytes, stream, &p);
  if (e) return e;
  return run_slice(p, row + p.a.out_r0, in, out);
}

extern "C" int thz_asm_slice_adjoint_workspace_size(const thz_asm_desc* d, size_t* bytes) {
  return asm_workspace_size(d, Pipe::SliceAdjoint, bytes);
}

extern "C" int thz_asm_slice_adjoint(const thz_asm_desc* d, int row, const void* grad_out, void* grad_in,
                                     void* workspace, size_t workspace_bytes, thz_stream_t stream) {
  AsmPlan p;
  int e = asm_plan(d, Pipe::SliceAdjoint, row, grad_out && grad_in, workspace, workspace_bytes, stream, &p);
  if (e) return e;
  return run_slice_adjoint(p, row + p.a.in_r0, grad_out, grad_in);
}

extern "C" int thz_asm_row_pairs(int mode) {
  if (mode < -1 || mode > 1) return fail(THZ_E_ARG, "thz_asm_row_pairs: mode %d (-1, 0 or 1)", mode);
  g_row_pairs.store(mode, std::memory_order_relaxed);
  return THZ_OK;
}

extern "C" int thz_asm_band(const thz_asm_desc* d, int* ncols, int* z_chunk) {
  int e = validate(d);
  if (e) return e;
  AsmGeom g;
  geometry(d, &g);
  if (ncols) *ncols = g.ncols;
  if (z_chunk) *z_chunk = g.zc;
  return THZ_OK;
}

extern "C" int thz_asm_workspace_size(const thz_asm_desc* d, size_t* bytes) {
  return asm_workspace_size(d, Pipe::Planes, bytes);
}

namespace thz {
// The optional parts of a planes pipeline; an empty one is thz_asm_forward.
struct AsmFused {
  // DOE modulation in K1's loader (desc null: none)
  struct {
    const thz_doe_desc* desc;
    const float *height, *noise;
    float* height_full;
  } mod{};
  const LossSink* loss = nullptr;  // the loss sums in K3's storer
  // the adjoint starts from the loss gradient at the stored forward output `field` (null: none)
  struct {
    const thz_loss_desc* desc;
    const float2* field;
    const float *target, *stats, *gloss;
  } grad{};
};

// the field a fused DOE modulates is the ASM input
static int check_doe_desc(const thz_asm_desc* d, const thz_doe_desc* m) {
  if (m->B != d->B || m->C != d->C || m->H != d->H || m->W != d->W)
    return fail(THZ_E_ARG, "DOE field %dx%dx%dx%d does not match the ASM input %dx%dx%dx%d", m->B, m->C, m->H, m->W,
                d->B, d->C, d->H, d->W);
  if (m->hs < 1 || m->ws < 1) return fail(THZ_E_ARG, "bad height-map size %dx%d", m->hs, m->ws);
  return THZ_OK;
}

// the field of a fused loss is the ASM output (Z B plane-major items), and the target broadcasts over it
static int check_loss_desc(const thz_asm_desc* d, const thz_loss_desc* l) {
  const int Ho = d->unpad ? d->H : d->H + 2 * d->pad_h, Wo = d->unpad ? d->W : d->W + 2 * d->pad_w;
  if (l->B != d->Z * d->B || l->C != d->C || l->H != Ho || l->W != Wo)
    return fail(THZ_E_ARG, "loss field %dx%dx%dx%d does not match the ASM output %dx%dx%dx%d", l->B, l->C, l->H, l->W,
                d->B, d->C, Ho, Wo);
  if (!(l->tB == 1 || l->tB == l->B) || !(l->tC == 1 || l->tC == l->C))
    return fail(THZ_E_ARG, "target %dx%d does not broadcast over %dx%d", l->tB, l->tC, l->B, l->C);
  return THZ_OK;
}

static int asm_forward_impl(const thz_asm_desc* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
                            thz_stream_t stream, const AsmFused& f) {
  AsmPlan p;
  int e = asm_plan(d, Pipe::Planes, 0, (in || f.grad.field) && out, workspace, workspace_bytes, stream, &p);
  if (e) return e;
  const AsmGeom& g = p.g;
  AsmArgs& a = p.a;
  if (const thz_doe_desc* m = f.mod.desc) {
    a.mod_h = f.mod.height;
    a.mod_u = f.mod.noise;
    a.mod_hfull = f.mod.height_full;
    a.mod_hs = m->hs;
    a.mod_ws = m->ws;
    a.mod_tol = m->tolerance;
    a.mod_eps = m->epsilon;
    a.mod_tand = m->tand;
    a.mod_rng = m->rng;
    a.mod_rng_stream = m->rng_stream;
  }
  if (d->window_mask) {
    const thz_aperture_desc* w = d->window_mask;
    const int Ho = d->adjoint ? g.Hin : g.Hout, Wo = d->adjoint ? g.Win : g.Wout;  // the forward's output grid
    if (w->kind != THZ_APERTURE_RECT && w->kind != THZ_APERTURE_CIRC)
      return fail(THZ_E_ARG, "window mask: bad aperture kind %d", w->kind);
    if (w->H != Ho || w->W != Wo)
      return fail(THZ_E_ARG, "window mask %dx%d does not match the output grid %dx%d", w->H, w->W, Ho, Wo);
    a.apm = aperture_args(w, Ho, Wo);
    a.ap_side = d->adjoint ? 2 : 1;
    // carried by the 300-point row passes only (the K3 storer forward, the K1 loader adjoint:
    // asm_rows_inv<300> / asm_rows_fwd<300>)
    if (g.Pw != Mx300::N)
      return fail(THZ_E_UNSUPPORTED, "window mask: only the 300-point row passes fold the aperture; "
                                     "apply it separately");
    if (d->adjoint && d->Z > 1)
      return fail(THZ_E_UNSUPPORTED, "window mask: one z-plane per adjoint call");
  }
  if (f.loss) a.ls = *f.loss;
  if (f.grad.field) {  // the adjoint pipeline starts from the loss gradient
    const thz_loss_desc* lg = f.grad.desc;
    a.lg_field = f.grad.field;
    a.lg_gloss = f.grad.gloss;
    a.lg_target = f.grad.target;
    a.lg_stats = f.grad.stats;
    a.lg_tB = lg->tB;
    a.lg_tC = lg->tC;
    // the loss of a Z-plane pipeline is the sum of the planes' means (thz_asm_forward_loss)
    a.lg_two_inv_n = (float)(2.0 * d->Z / ((double)lg->B * lg->C * lg->H * lg->W));
  }
  if (p.ws[2]) {  // the mixed-radix heights: the column pass's tables (tab_bytes: sqt, then mzt)
    a.sqt = (float*)p.ws[2];
    a.mzt = (int*)(p.ws[2] + tab_sq_bytes(g));
  }
  return run_pipeline(p, in, out);
}
}  // namespace thz

extern "C" int thz_asm_forward(const thz_asm_desc* d, const void* in, void* out, void* workspace,
                               size_t workspace_bytes, thz_stream_t stream) {
  return asm_forward_impl(d, in, out, workspace, workspace_bytes, stream, AsmFused{});
}

namespace thz {
// ASM_prop.create_kernel (Props/ASM_Prop.py:212-311): H of one z on the CENTRED grid of the padded
// plane, [C][Ph][Pw], the row i / column j at spectral index m = i - Ph/2 (:141-145).  The same
// fp32 scalars, masks and phase as the propagation kernels (tf_scalars / tf_value), so the table
// is exactly the transfer function they apply on the fly; only inspection reads it
// (ASM_prop.visualize_kernel).
__global__ void __launch_bounds__(256) asm_tf_export(float2* __restrict__ out, AsmArgs a) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, c = blockIdx.z;
  if (j >= a.Pw) return;
  const TfScalars s = tf_scalars(a, a.lam[c], a.zv[0]);
  const float Kx = kfreq(i - a.Ph / 2, a.Ph, a.dx), Ky = kfreq(j - a.Pw / 2, a.Pw, a.dy);
  out[((size_t)c * a.Ph + i) * a.Pw + j] = tf_value(a, s, Kx, Ky);
}
}  // namespace thz

extern "C" int thz_asm_transfer_function(const thz_asm_desc* d, void* out, thz_stream_t stream) {
  int e = validate(d);
  if (e) return e;
  if (!out) return fail(THZ_E_ARG, "null output pointer");
  if (!d->z) return fail(THZ_E_ARG, "the transfer-function table takes a host z");
  AsmGeom g;
  geometry(d, &g);
  AsmArgs a = asm_args_base(d, g);
  a.adjoint = 0;  // the table is H itself whatever the descriptor's direction
  hipStream_t s = (hipStream_t)stream;
  KernelTimer kt("asm_tf_export", s);
  hipLaunchKernelGGL(asm_tf_export, dim3((g.Pw + 255) / 256, g.Ph, d->C), dim3(256), 0, s, (float2*)out, a);
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_asm_forward_modulated(const thz_asm_desc* d, const thz_doe_desc* m, const void* field,
                                         const float* height, const float* noise, float* height_full, void* out,
                                         void* workspace, size_t workspace_bytes, thz_stream_t stream) {
  if (!d || !m || !height) return fail(THZ_E_ARG, "null descriptor / height");
  if (d->adjoint) return fail(THZ_E_ARG, "the fused DOE modulation is forward only");
  int e = check_doe_desc(d, m);
  if (e) return e;
  AsmFused f;
  f.mod = {m, height, noise, height_full};
  return asm_forward_impl(d, field, out, workspace, workspace_bytes, stream, f);
}

extern "C" int thz_asm_adjoint_loss(const thz_asm_desc* d, const thz_loss_desc* l, const void* field,
                                     const float* target, const float* stats, const float* grad_loss,
                                     const void* grad_out, void* grad_in, void* workspace, size_t workspace_bytes,
                                     thz_stream_t stream) {
  int e = validate(d);
  if (e) return e;
  if (!l || !field || !target || !stats || !grad_loss || !grad_in)
    return fail(THZ_E_ARG, "null loss descriptor / field / target / stats / grad_loss / grad_in");
  if (!d->adjoint) return fail(THZ_E_ARG, "the fused loss adjoint takes adjoint == 1");
  if ((e = check_loss_desc(d, l))) return e;
  AsmFused f;
  f.grad = {l, (const float2*)field, target, stats, grad_loss};
  return asm_forward_impl(d, grad_out, grad_in, workspace, workspace_bytes, stream, f);
}

extern "C" int thz_asm_forward_loss(const thz_asm_desc* d, const thz_doe_desc* m, const void* field,
                                    const float* height, const float* noise, float* height_full,
                                    const thz_loss_desc* l, const float* target, void* out, float* loss, float* stats,
                                    void* workspace, size_t workspace_bytes, thz_stream_t stream) {
  int e = validate(d);
  if (e) return e;
  if (!l || !target || !loss || !stats) return fail(THZ_E_ARG, "null loss descriptor / target / loss / stats");
  if (d->adjoint) return fail(THZ_E_ARG, "the fused loss is forward only (thz_asm_adjoint_loss)");
  if ((e = check_loss_desc(d, l))) return e;
  AsmFused f;
  if (m) {
    if (!height) return fail(THZ_E_ARG, "null height map");
    if ((e = check_doe_desc(d, m))) return e;
    f.mod = {m, height, noise, height_full};
  }
  const LossSink ls = loss_sink(l, target, loss, stats, l->C * l->H, d->Z);
  f.loss = &ls;
  return asm_forward_impl(d, field, out, workspace, workspace_bytes, stream, f);
}

namespace thz {
// rows transforms of length n, row r at in/out + r * stride (in place allowed): one launch
int fft_rows_strided(const void* in, void* out, int rows, int n, size_t stride, int inverse, hipStream_t s) {
  if (!in || !out || rows < 1 || stride < (size_t)n) return fail(THZ_E_ARG, "bad fft_rows arguments");
  FftPlan p;
  int e = get_plan(n, &p);
  if (e) return e;
  if ((e = ensure_lds_attr())) return e;
  on_pow2(n, [&](auto N) {
    hipLaunchKernelGGL(fft_rows_kernel<N()>, dim3(rows), dim3(threads_for(n)), fft_lds_bytes_io(n), s,
                       (const float2*)in, (float2*)out, p, inverse, stride);
  });
  THZ_LAUNCH_CHECK();
  return THZ_OK;
}
}  // namespace thz

extern "C" int thz_fft_rows(const void* in, void* out, int rows, int n, int inverse, thz_stream_t stream) {
  return fft_rows_strided(in, out, rows, n, (size_t)n, inverse, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// RSC / VRS C-ABI
// ---------------------------------------------------------------------------------------------
namespace thz {

struct RscPlan {
  AsmGeom g;
  RscKArgs k;
  size_t tk, kf, t, u;  // byte sizes: the kernel's row pass | its spectrum (a.tft) | T | U
  size_t total() const { return tk + kf + t + u; }
};

// The shape rules of the RSC entry points (the planes, and thz_rsc.hip's z-x slice): the doubled grid Ph x Pw.
int rsc_shape(int B, int C, int H, int W, int vectorial, const float* wavelengths, int* Ph, int* Pw) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return fail(THZ_E_ARG, "bad RSC shape");
  if (vectorial && B < 2) return fail(THZ_E_ARG, "vectorial RSC needs Ex, Ey planes (B >= 2)");
  if (C > THZ_MAX_WAVELENGTHS) return fail(THZ_E_UNSUPPORTED, "C=%d > %d", C, THZ_MAX_WAVELENGTHS);
  if (!wavelengths) return fail(THZ_E_ARG, "null wavelengths");
  *Ph = H + 2 * (H / 2);
  *Pw = W + 2 * (W / 2);
  if (*Ph > FFT_MAX_N || *Pw > FFT_MAX_N) return fail(THZ_E_UNSUPPORTED, "RSC grid %dx%d too large", *Ph, *Pw);
  return THZ_OK;
}

static int rsc_plan(const thz_rsc_desc* d, RscPlan* p) {
  if (!d) return fail(THZ_E_ARG, "null descriptor");
  AsmGeom& g = p->g;
  int e = rsc_shape(d->B, d->C, d->H, d->W, d->vectorial, d->wavelengths, &g.Ph, &g.Pw);
  if (e) return e;
  g.BC = (d->vectorial ? 3 : d->B) * d->C;
  if (d->adjoint && d->vectorial) return fail(THZ_E_ARG, "RSC adjoint is per plane: vectorial must be 0");
  g.Hin = d->adjoint ? g.Ph - d->H : d->H;
  g.Win = d->adjoint ? g.Pw - d->W : d->W;
  g.Hout = d->adjoint ? d->H : g.Ph - d->H;  // ifft2(...)[..., H:, W:] (:207)
  g.Wout = d->adjoint ? d->W : g.Pw - d->W;
  g.ncols = g.Pw;
  g.J = g.Pw / 2;
  g.ncb = (g.ncols + CB - 1) / CB;
  g.ncbu = (g.ncols + CBU - 1) / CBU;
  g.zc = 1;
  g.adj = 0;
  g.C = d->C;
  RscKArgs& k = p->k;
  k.C = d->C;
  k.Ph = g.Ph;
  k.Pw = g.Pw;
  k.ncbK = g.ncb;
  k.dx = d->dx;
  k.z = d->z;
  for (int c = 0; c < d->C; ++c) k.lam[c] = d->wavelengths[c];
  p->tk = align256((size_t)d->C * k.ncbK * CB * g.Ph * sizeof(float2));
  p->kf = align256((size_t)d->C * g.Pw * g.Ph * sizeof(float2));
  p->t = t_bytes(g);
  p->u = u_bytes(g, 1);
  return THZ_OK;
}

}  // namespace thz

extern "C" int thz_rsc_workspace_size(const thz_rsc_desc* d, size_t* bytes) {
  RscPlan p;
  int e = rsc_plan(d, &p);
  if (e) return e;
  if (!bytes) return fail(THZ_E_ARG, "null bytes");
  *bytes = p.total();
  return THZ_OK;
}

extern "C" int thz_rsc_forward(const thz_rsc_desc* d, const void* in, void* out, void* workspace,
                               size_t workspace_bytes, thz_stream_t stream) {
  RscPlan p;
  int e = rsc_plan(d, &p);
  if (e) return e;
  if (!in || !out) return fail(THZ_E_ARG, "null data pointer");
  if ((e = check_workspace(workspace, workspace_bytes, p.total()))) return e;
  AsmPlan ap;
  ap.g = p.g;
  const AsmGeom& g = ap.g;
  if ((e = device_plans(g, &ap.pw, &ap.ph))) return e;
  hipStream_t s = ap.s = (hipStream_t)stream;
  char* w = (char*)workspace;
  float2* TK = (float2*)w;
  float2* KF = (float2*)(w + p.tk);
  ap.ws[0] = w + p.tk + p.kf;         // T
  ap.ws[1] = w + p.tk + p.kf + p.t;   // U
  ap.ws[2] = nullptr;                 // no column tables: the transfer function is KF
  ap.Z = 1;
  {
    KernelTimer kt("rsc_kernel_fft", s);
    on_pow2(g.Pw, [&](auto N) {
      hipLaunchKernelGGL(rsc_k_rows<N()>, dim3(d->C * g.Ph), dim3(threads_for(g.Pw)), fft_lds_bytes_io(g.Pw), s, TK,
                         ap.pw, p.k);
    });
    THZ_LAUNCH_CHECK();
    on_pow2(g.Ph, [&](auto N) {
      hipLaunchKernelGGL(rsc_k_cols<N()>, dim3(d->C * g.Pw), dim3(threads_for(g.Ph)), fft_lds_bytes_io(g.Ph), s,
                         (const float2*)TK, KF, ap.ph, p.k);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  // the shared base, then what the convolution changes: its windows in the doubled plane, no band
  // limit, the quadrature weight in the scale, the kernel's spectrum as the transfer function, Ez
  AsmArgs& a = ap.a = args_base(g, THZ_BANDLIMIT_NONE, d->dx, d->dy, d->wavelengths);
  if (!d->adjoint) {  // U[..., :H, :W] = field (:198-200), read back from [H:, W:]
    a.out_r0 = d->H; a.out_c0 = d->W;
  } else {  // adjoint: gradient placed at [H:, W:], result read back from [:H, :W]
    a.in_r0 = d->H; a.in_c0 = d->W;
    a.adjoint = 1;
  }
  a.scale = (float)((double)d->dx * (double)d->dy / ((double)g.Ph * (double)g.Pw));
  a.tft = KF;
  a.vec = d->vectorial;
  a.zr = d->z;
  a.zv[0] = d->z;
  return run_pipeline(ap, in, out);
}
