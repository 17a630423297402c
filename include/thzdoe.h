/*
 * thzdoe.h -- C-ABI of libthzdoe.so, the MI355X (gfx950) hot path of
 * QuantizationAwareTHzDOE: band-limited angular-spectrum (ASM), chirp-z (CZT) and
 * Rayleigh-Sommerfeld (RSC) complex-field propagators and the quantized-DOE phase
 * modulation.
 *
 * Conventions (all entry points):
 *   - extern "C", C types only; no exception crosses the boundary.
 *   - every entry returns int: THZ_OK (0) or a THZ_E_* code; thz_last_error()
 *     returns a thread-local message describing the last failure.
 *   - complex data is interleaved (re, im) float32, i.e. the memory of
 *     torch.complex64; all data/workspace pointers are DEVICE pointers owned by
 *     the caller (PyTorch's caching allocator).  The library allocates nothing per
 *     call; it keeps immutable per-device twiddle tables built lazily under a mutex
 *     (so the first call for a new length must not be inside a stream capture).
 *   - calls enqueue asynchronously on `stream` and never synchronise the device.
 *   - per-call physical scalars (wavelengths, z) are HOST arrays; they travel as
 *     kernel arguments, so calls are hipGraph-capturable after warm-up.
 *
 * Reference interfaces replaced (paths relative to the reference repo root):
 *   thz_asm_*        Props/ASM_Prop.py:17-378    ASM_prop.forward (+ autograd adjoint)
 *   thz_czt_*        Props/CZT_Prop.py:11-314    CZT_prop.forward / VCZT_prop
 *   thz_rsc_*        Props/RSC_Prop.py:15-321    RSC_prop.forward / VRS_prop.forward
 *   thz_doe_*        Components/QuantizedDOE.py:44-126  DOELayer.modulate (+ backward)
 *   thz_quant_*      Components/QuantizedDOE.py:181-1388 quantized height maps (+ backward)
 *   thz_fft_*        utils/Helper_Functions.py:99-160 ft2/ift2 (centred ortho FFT)
 *   thz_stokes_*, thz_polarization_ellipse*  Addons/Polarization.py:45-92  PolarizationAnalyser
 *   thz_noise_*, thz_signal_scale*, thz_snr_noise_backward  Addons/Noise.py:4-112, utils/Noise.py:4-116,
 *                    utils/Helper_Functions.py:258-366  the detector noise models
 */
#ifndef THZDOE_H_
#define THZDOE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define THZ_OK 0
#define THZ_E_ARG 1         /* invalid argument / shape */
#define THZ_E_UNSUPPORTED 2 /* size outside what the kernels support */
#define THZ_E_WORKSPACE 3   /* workspace too small */
#define THZ_E_HIP 4         /* HIP runtime error (message in thz_last_error) */

#define THZ_BANDLIMIT_NONE 0
#define THZ_BANDLIMIT_EXACT 1  /* Matsushima eqs. 18-19, Props/ASM_Prop.py:296-301 */
#define THZ_BANDLIMIT_APPROX 2 /* Matsushima eqs. 21-22, Props/ASM_Prop.py:302-306 */

#define THZ_MAX_WAVELENGTHS 64
#define THZ_MAX_Z 256

typedef void* thz_stream_t; /* hipStream_t */

/* ABI of this header.  Bumped whenever a descriptor struct changes layout (round 2 appended
 * rng / rng_stream to thz_doe_desc and thz_quant_desc; 4 added thz_asm_transfer_function and
 * thz_rs_kernel, which the bindings require; 5 appended thz_asm_desc.window_mask, 6 thz_asm_desc.z_dev,
 * 7 added thz_doe_quant_backward and thz_radial_quant_backward, 8 thz_step_fetch and
 * thz_adam_step, 9 thz_asm_slice_workspace_size and thz_asm_slice_forward;
 * thz_asm_slice_adjoint_workspace_size and thz_asm_slice_adjoint (library 0.6.0) changed no struct and
 * are purely additive, so the version stays 9 -- a caller detects them by symbol; likewise
 * thz_czt_slice_workspace_size and thz_czt_slice_forward with their own new thz_czt_slice_desc, and
 * thz_czt_slice_adjoint_workspace_size and thz_czt_slice_adjoint on the same descriptor, and
 * thz_rsc_slice_workspace_size and thz_rsc_slice_forward with their new thz_rsc_slice_desc, and
 * thz_rsc_slice_adjoint_workspace_size and thz_rsc_slice_adjoint on the same descriptor, and the
 * descriptor-free polarization entries thz_stokes_forward, thz_stokes_backward,
 * thz_polarization_ellipse, thz_stokes64_forward and thz_polarization_ellipse64, and the noise
 * entries thz_noise_apply (with its new thz_noise_desc), thz_noise_draws,
 * thz_signal_scale_workspace_size, thz_signal_scale and thz_snr_noise_backward, and the metrics entries
 * thz_region_stats_workspace_size, thz_region_stats_forward, thz_region_stats_backward (with their new
 * thz_region_stats_desc) and thz_line_widths):
 * a caller compares thz_abi_version()
 * with the THZ_ABI_VERSION it was compiled against before its first call, since a shorter
 * struct from an older header would make the library read past it.  Descriptors are plain C
 * structs: zero-initialise them (memset / `= {0}` / ctypes defaults) so fields a caller does not
 * know about stay 0 (no noise buffer and no device generator means no noise). */
#define THZ_ABI_VERSION 9

/* Library identity. */
const char* thz_version(void);
const char* thz_last_error(void);
int thz_abi_version(void);

/*
 * Angular-spectrum propagation, Props/ASM_Prop.py:314-378 (forward) and its
 * adjoint (autograd backward, == ASM with conj(H)).
 *
 * Forward : in  [B, C, H, W]     -> out [Z, B, C, Ho, Wo]
 * Adjoint : in  [Z, B, C, Ho, Wo] -> out [B, C, H, W] = sum over z of plane z's adjoint (the
 *           autograd backward of a Z-plane forward; the column pass sums the planes' spectra,
 *           one inverse column transform and one row pass in all)
 * with Ho = H, Wo = W when unpad != 0 (CenterCrop, :359-361) else Ho = H+2 pad_h,
 * Wo = W + 2 pad_w (do_unpad_after_pad=False).  pad_h = floor(s_h H / 2) as in
 * compute_padding (:119-136); do_padding=False is pad_h = pad_w = 0.
 * wavelengths[C] and z[Z] are host float arrays (metres); dx, dy = field.spacing.
 */
typedef struct thz_asm_desc {
  int B, C, H, W;
  int pad_h, pad_w;
  int unpad;
  int bandlimit;            /* THZ_BANDLIMIT_* */
  int Z;                    /* 1 .. THZ_MAX_Z */
  int adjoint;              /* 0 forward, 1 adjoint (sums the Z planes) */
  int z_chunk;              /* z-planes per column pass; 0 = library default */
  float dx, dy;
  const float* wavelengths; /* host [C] */
  const float* z;           /* host [Z] */
  /* optional (NULL = none, ABI 5): an aperture on the output grid (ApertureElement after ASM_prop,
   * Components/Aperture.py:104-136, e.g. the DONN's layers, experiment_DONN_3_layers.ipynb:109-200),
   * applied in the row-inverse pass's stores (forward) or in the row pass's loads of the adjoint's
   * input (the adjoint of mask * ASM is ASM^H * mask).  Its BC is ignored; H, W must be the
   * output grid's (unpad ? H, W : the padded plane); the field is multiplied by 1 / 0, so NaN / inf
   * propagate as in the reference's field * mask.  Carried by the 300-point padded row length only
   * (the DONN / QAT layer geometry); other geometries return THZ_E_UNSUPPORTED (apply
   * thz_aperture separately), as does an adjoint with Z > 1. */
  const struct thz_aperture_desc* window_mask;
  /* optional (NULL = none, ABI 6): the Z plane distances in DEVICE memory [Z], read by the kernels
   * in place of z[] -- a captured HIP graph then replays with whatever the caller writes there
   * before each replay (the extended-depth-of-focus loop re-draws its five planes every iteration,
   * experiment_extend_depth_of_focus.ipynb cell 22).  The spectral band is then sized for any z
   * (the evanescent bound |Ky| <= k; the band limit still masks per element), and z[] (host) may be
   * NULL.  The caller keeps the values fixed between a forward and its adjoint. */
  const float* z_dev;
} thz_asm_desc;

/* Workspace: the row-pass spectrum T [BC][ncols][H], one z-chunk of column-pass output
 * U [zc][BC][ncols][Ho] (both complex64; the adjoint holds a z-chunk of input planes in T,
 * [zc][BC][ncols][Ho], and one summed plane in U), and for a 300-point padded height the
 * mixed-radix column pass's per-(wavelength, column) tables (sqrt row values and
 * kept-row bounds).  Contents need not persist between calls. */
int thz_asm_workspace_size(const thz_asm_desc* d, size_t* bytes);
int thz_asm_forward(const thz_asm_desc* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
                    thz_stream_t stream);
/*
 * z-x slice: one output row of every plane of a z-sweep, without forming the planes -- the axial
 * map of experiment_extend_depth_of_focus.ipynb:229-263 (cell Submm_Setup_test.forward: for each z
 * of prop_range = np.linspace(20 mm, 120 mm, num=200) it propagates the whole plane and keeps
 * final_field.data[0, 0, 49, :], stacked into fields_zx).
 *   in [B, C, H, W] -> out [Z, B, C, Wo] == thz_asm_forward's out[:, :, :, row, :]
 * row indexes the output grid, 0 <= row < Ho (Ho = H when unpad is set, else the padded height).
 * The row pass runs as in thz_asm_forward; the column pass folds exp(2 pi i m R / Ph) of the padded
 * row R into the column spectrum once and then sums spectrum x H_z per plane (no inverse column
 * transform, no per-plane intermediate of height Ho); one Pw-point inverse row transform per
 * (z, b, c).  Forward only (its adjoint is thz_asm_slice_adjoint below), host z[] only, no window mask: adjoint != 0, z_dev != NULL and
 * window_mask != NULL return THZ_E_UNSUPPORTED, as does a padded height H + 2 pad_h other than
 * 1024, 2048, 4096, 8192 or 16384 (slice thz_asm_forward's planes there); a bad row or a null
 * pointer THZ_E_ARG; a short workspace THZ_E_WORKSPACE -- all before any device call.
 * Workspace: T as above and V [zc][BC][ncols] complex64, the column sums of zc = min(64, the forward's
 * z-chunk) planes at a time (the plane recurrence restarts with every chunk, as in thz_asm_forward).
 */
int thz_asm_slice_workspace_size(const thz_asm_desc* d, size_t* bytes);
int thz_asm_slice_forward(const thz_asm_desc* d, int row, const void* in, void* out /* [Z,B,C,Wo] */,
                          void* workspace, size_t workspace_bytes, thz_stream_t stream);
/*
 * Adjoint of the z-x slice (the autograd backward of thz_asm_slice_forward; library 0.6.0):
 *   grad_out [Z, B, C, Wo] -> grad_in [B, C, H, W] = sum over z of A_{z,row}^H grad_out[z]
 * d is the forward's descriptor with adjoint == 1 (anything else: THZ_E_ARG); row as in the forward.
 * One forward Pw-point row transform per (z, b, c) (asm_rows_fwd on one-row planes), one column pass
 * that sums conj(H_z) x the rows' spectra over all Z planes in registers (the forward's band, plane
 * recurrence and step factors, conjugated; a fresh sincos anchor at least every 64 planes) and
 * inverts once per column, and the adjoint's usual inverse row pass (asm_rows_inv).  Two calls with
 * the same inputs are bit-identical (fixed summation order, no atomics).  Validation as the
 * forward's, before any device call: z_dev, window_mask and a padded height outside the five powers
 * of two THZ_E_UNSUPPORTED; a bad row or a null pointer THZ_E_ARG; a short workspace THZ_E_WORKSPACE.
 * Workspace: the gradient spectrum of ONE plane [BC][ncols][H] and the rows' spectra
 * Gv [Z][BC][ncols rounded up to 16], both complex64 -- nothing of a plane's size per z.
 */
int thz_asm_slice_adjoint_workspace_size(const thz_asm_desc* d, size_t* bytes);
int thz_asm_slice_adjoint(const thz_asm_desc* d, int row, const void* grad_out /* [Z,B,C,Wo] */,
                          void* grad_in /* [B,C,H,W] */, void* workspace, size_t workspace_bytes,
                          thz_stream_t stream);
/* Plan facts for diagnostics / bench byte counts: number of spectral columns the kernels
 * keep (|m_y| <= J; ncols = 2J+1, or Pw when nothing is cut) and z-planes per column pass. */
int thz_asm_band(const thz_asm_desc* d, int* ncols, int* z_chunk);
/* Diagnostics (process-wide, like thz_timing_enable; purely additive, THZ_ABI_VERSION stays 9): which
 * form of the inverse row pass the plain power-of-two ASM pipelines run from the next call on.
 *   -1 the library's choice (the default: row pairs where they were measured faster, the middle-half
 *      crop of a 8192-point row), 0 one output row per workgroup, 1 two rows per workgroup at every
 *      power-of-two row length 1024 .. 16384.
 * Both forms give bit-identical planes (tests/test_asm_rows_pair_gpu.py compares them); the fused-loss
 * and mixed-radix row passes have one form and ignore the setting.  Another mode: THZ_E_ARG. */
int thz_asm_row_pairs(int mode);
/* The transfer function the ASM kernels apply on the fly, materialised for inspection:
 * ASM_prop.create_kernel (Props/ASM_Prop.py:212-311; used by visualize_kernel, :198-210).
 * out [C, Ph, Pw] complex64 (device) on the CENTRED frequency grid of the padded plane
 * (row i <-> Kx = 2 pi ((i - Ph/2) / Ph) / dx, :141-145, 244-245), H = exp(i z sqrt(k^2 - K^2))
 * with the evanescent cut (:262) and the desc's band limit (:264-309), z = d->z[0].
 * Uses C, H, W, pad_h, pad_w, bandlimit, dx, dy, wavelengths, z of the descriptor. */
int thz_asm_transfer_function(const thz_asm_desc* d, void* out, thz_stream_t stream);

/*
 * Chirp-z (Bluestein) Rayleigh-Sommerfeld propagation with output zoom,
 * Props/CZT_Prop.py:252-314 (forward).
 *   in  [B, C, H, W] complex64, spacing (dx, dy)
 *   out [B, C, outW, outH] (the reference's transposed result; outH must equal outW,
 *        as the reference's final F0 * U broadcast requires, :248)
 * wavelengths[C] host floats; z, output spacing (odx, ody) as in forward(field, outputHeight,
 * outputWidth, outputPixel_dx, outputPixel_dy).
 * THZ_E_ARG when H + outW - 1 or W + outH - 1 is a power of two: the reference's Bluestein
 * slice keeps one row too few there and raises (Props/CZT_Prop.py:206,211).
 */
typedef struct thz_czt_desc {
  int B, C, H, W;
  int outH, outW;
  float dx, dy;
  float odx, ody;
  float z;
  const float* wavelengths; /* host [C] */
  int adjoint;              /* 1: the adjoint (autograd backward): in [B, C, outW, outH] ->
                               out [B, C, H, W]; conj chirps / filter / RS kernels, passes reversed */
} thz_czt_desc;

int thz_czt_workspace_size(const thz_czt_desc* d, size_t* bytes);
int thz_czt_forward(const thz_czt_desc* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
                    thz_stream_t stream);

/*
 * CZT z-x slice: one zoomed output row of every plane of a z-sweep, without forming the planes --
 * the x-z cross-section of a focal region on the zoomed grid (Props/CZT_Prop.py:227-314 called once
 * per plane, keeping out[..., row, :]; :260-262 "useful for imaging light in the focal plane: allows
 * high resolution zoom").  Purely additive (no struct changed): THZ_ABI_VERSION stays 9, a caller
 * detects the entries by symbol.
 *   in [B, C, H, W] -> out [Z, B, C, outH] == thz_czt_forward(z = z[k])'s out[:, :, row, :] for every k
 * row is the p of out[b, c, p, q], 0 <= row < outW.  For a fixed p the pass along H is a dot product
 * per input column: a collapse kernel forms S_k[b,c,w] = sum_h in[b,c,h,w] F_{z_k,c}(x_h, y_w)
 * preB[h] gB[p + H - h] for four planes per read of the field, then one W-axis Bluestein line of
 * np2 = 2^ceil(log2(W + outH - 1)) points per (k, b, c).  No intermediate of a plane's size, no
 * second pass, no per-z table cache; two calls with the same inputs are bit-identical (H is split in
 * a fixed way and its partial sums are added in order, no atomics).  Forward only (its adjoint is
 * thz_czt_slice_adjoint below), host z[] only.
 * Validation, all before any device call: the shape rules of thz_czt_forward (square output,
 * C <= THZ_MAX_WAVELENGTHS, THZ_E_ARG for a power-of-two Bluestein length, THZ_E_UNSUPPORTED past the
 * longest transform); a bad row, Z outside 1 .. THZ_MAX_Z or a null pointer THZ_E_ARG; a short or
 * null workspace THZ_E_WORKSPACE (the message names the size).
 * Workspace, with zc = min(Z, 16) planes per chunk and r32(n) = n rounded up to 32:
 *   8 zc C (r32(W) + r32(outH) + np2 + r32(H) + 32)     tables per (plane, wavelength)
 * + 8 hs zc B C W                                        S, in hs <= 8 partial sums over H
 * bytes, each part rounded up to 256 -- nothing of size H x outH or outW x outH, and no growth with
 * Z past one chunk.
 */
typedef struct thz_czt_slice_desc {
  int B, C, H, W;
  int outH, outW;
  float dx, dy, odx, ody;
  int Z;                    /* 1 .. THZ_MAX_Z */
  const float* z;           /* host [Z] */
  const float* wavelengths; /* host [C] */
  int row;                  /* 0 <= row < outW: the p of out[b, c, p, q] */
} thz_czt_slice_desc;

int thz_czt_slice_workspace_size(const thz_czt_slice_desc* d, size_t* bytes);
int thz_czt_slice_forward(const thz_czt_slice_desc* d, const void* in /* [B,C,H,W] */,
                          void* out /* [Z,B,C,outH] */, void* workspace, size_t workspace_bytes,
                          thz_stream_t stream);
/*
 * Adjoint of the CZT z-x slice (the autograd backward of thz_czt_slice_forward), same descriptor:
 *   grad_out [Z, B, C, outH] -> grad_in [B, C, H, W] = sum over k of A_{z_k,row}^H grad_out[k]
 * Per chunk of 16 planes, with the forward's tables: one W-axis Bluestein line per (k, b, c) in the
 * adjoint form (conjugated chirps, filter spectrum and F0; windows exchanged) gives
 * T_k[b,c,w], then an expand kernel adds sum_k conj(F_{z_k,c}(x_h, y_w) coef_kc[h]) T_k[b,c,w] to
 * grad_in[b,c,h,w] -- one RS-kernel evaluation per (element, plane), as the forward's collapse.  The
 * first chunk stores grad_in (it may be uninitialised memory; every element is written), later chunks
 * read, add and store it on the same stream: no memset, no atomics, a fixed summation order, so two
 * calls with the same inputs are bit-identical.  Purely additive: THZ_ABI_VERSION stays 9, a caller
 * detects the entries by symbol.  Validation as the forward's, all before any device call: a bad
 * row, Z outside 1 .. THZ_MAX_Z or a null pointer THZ_E_ARG; a short or null workspace
 * THZ_E_WORKSPACE (the message names the size).
 * Workspace, with zc = min(Z, 16) and r32 as above:
 *   8 zc C (r32(W) + r32(outH) + np2 + r32(H) + 32)     tables per (plane, wavelength)
 * + 8 zc B C W                                           T
 * bytes, each part rounded up to 256 -- nothing of a plane's size, no growth with Z past one chunk.
 */
int thz_czt_slice_adjoint_workspace_size(const thz_czt_slice_desc* d, size_t* bytes);
int thz_czt_slice_adjoint(const thz_czt_slice_desc* d, const void* grad_out /* [Z,B,C,outH] */,
                          void* grad_in /* [B,C,H,W] */, void* workspace, size_t workspace_bytes,
                          thz_stream_t stream);

/*
 * Rayleigh-Sommerfeld convolution, Props/RSC_Prop.py:170-215 (RSC_prop.forward), and its
 * vectorial form VRS_prop.forward (:265-321, vectorial != 0: planes 0/1 of the input are
 * Ex/Ey, Ez = (Ex x + Ey y)/r is formed in the kernel, output has 3 planes).
 *   in  [B, C, H, W] -> out [Bo, C, Ph - H, Pw - W], Ph = H + 2 floor(H/2) (the reference's
 *   ifft2(...)[..., H:, W:] window, :207), Bo = vectorial ? 3 : B.
 * The spatial kernel grid uses dx on both axes (:83-84) and the spectrum is scaled by dx*dy.
 */
typedef struct thz_rsc_desc {
  int B, C, H, W;
  int vectorial;
  float dx, dy;
  float z;
  const float* wavelengths; /* host [C] */
  int adjoint;              /* 1: the adjoint (autograd backward) of the scalar convolution:
                               in [B, C, Ph - H, Pw - W] -> out [B, C, H, W], conj(FFT2(K)),
                               windows exchanged; vectorial must be 0 (VRS backward applies it
                               per plane and folds the Ez chain on the host side) */
} thz_rsc_desc;

int thz_rsc_workspace_size(const thz_rsc_desc* d, size_t* bytes);
int thz_rsc_forward(const thz_rsc_desc* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
                    thz_stream_t stream);

/*
 * RSC / VRS z-x slice: one output row of every plane of a z-sweep, without forming the planes -- the
 * x-z cross-section of a focal region on the Rayleigh-Sommerfeld convolution (Props/RSC_Prop.py:170-215,
 * vectorial :265-321, called once per plane keeping out[..., row, :]).  Purely additive (no struct
 * changed): THZ_ABI_VERSION stays 9, a caller detects the entries by symbol.
 *   in [B, C, H, W] -> out [Z, Bo, C, Pw - W] == thz_rsc_forward(z = z[k])'s out[:, :, row, :] for every k
 * row indexes the output window, 0 <= row < Ph - H.  With x = linspace(-Ph dx/2, Ph dx/2, Ph),
 * y = linspace(-Pw dx/2, Pw dx/2, Pw) (dx on both axes, :83-84) the 2-D circular convolution at output
 * row H + row is a sum of H one-dimensional ones, and it never wraps (1 <= H + row - i <= Ph - 1):
 *   out[k,b,c,q] = dx dy IFFT_Pw( sum_{i<H} FFT_Pw(in[b,c,i,:] zero-padded)[m]
 *                                           FFT_Pw(RS_{z_k,c}(x[H + row - i], y[:]))[m] )[W + q]
 * The input rows' spectra Uh are formed once per call (they do not depend on z; VRS's Ez does,
 * through r = sqrt(x^2 + y^2 + z^2) of :294-303, so its rows are formed per plane of the chunk); a
 * kernel row's spectrum serves every b.  Per chunk of zc = min(Z, 32) planes one accumulate launch
 * (kernel row -> Pw-point transform in LDS -> x Uh -> partial sums over hs fixed splits of the input
 * rows, in registers) and one line launch (the hs partials added in index order, one inverse Pw-point
 * transform per (k, b, c), x dx dy / Pw, elements [W, Pw)).  No transform along H, no Ph x Pw kernel
 * table or its 2-D FFT; two calls with the same inputs are bit-identical (fixed split, fixed order,
 * no atomics).  Forward only (the adjoint is thz_rsc_slice_adjoint below), host z[] only.
 * Validation, all before any device call: the shape rules of thz_rsc_forward (THZ_E_ARG for a bad
 * shape, vectorial with B < 2 or null wavelengths; THZ_E_UNSUPPORTED for C > THZ_MAX_WAVELENGTHS or a
 * grid past the longest transform); a bad row, Z outside 1 .. THZ_MAX_Z or a null pointer THZ_E_ARG; a
 * short or null workspace THZ_E_WORKSPACE (the message names the size).
 * Workspace, with hs = max(1, min(H, 64, floor(2048 / (32 C)))) (a function of H and C alone, so a
 * plane is summed alike whatever batch it is part of):
 *   8 (vectorial ? 2 + zc : B) C H Pw      Uh, the input rows' spectra
 * + 8 zc Bo C hs Pw                        P, one chunk's partial sums
 * bytes, each part rounded up to 256 -- no Ph x Pw table, no growth with Z past one chunk.
 */
typedef struct thz_rsc_slice_desc {
  int B, C, H, W;
  int vectorial;            /* as thz_rsc_desc: planes 0/1 are Ex/Ey, 3 planes out */
  float dx, dy;
  int Z;                    /* 1 .. THZ_MAX_Z */
  const float* z;           /* host [Z] */
  const float* wavelengths; /* host [C] */
  int row;                  /* 0 <= row < Ph - H */
} thz_rsc_slice_desc;

int thz_rsc_slice_workspace_size(const thz_rsc_slice_desc* d, size_t* bytes);
int thz_rsc_slice_forward(const thz_rsc_slice_desc* d, const void* in /* [B,C,H,W] */,
                          void* out /* [Z,Bo,C,Pw-W] */, void* workspace, size_t workspace_bytes,
                          thz_stream_t stream);
/*
 * Adjoint of the RSC / VRS z-x slice (the autograd backward of thz_rsc_slice_forward), same descriptor:
 *   grad_out [Z, Bo, C, Pw - W] -> grad_in [B, C, H, W] = sum over k of A_{z_k,row}^H grad_out[k]
 * With Kh_{k,c,i} = FFT_Pw(RS_{z_k,c}(x[H + row - i], y[:])), the forward's kernel rows, per chunk of
 * zc = min(Z, 32) planes:
 *   Gh[k,b,c,:]  = dx dy / Pw FFT_Pw(grad_out[k,b,c,:] placed at [W, Pw), zeros before)   one line per (k, b, c)
 *   S[b,c,i,m]  += sum over the chunk's k of conj(Kh_{k,c,i}[m]) Gh[k,b,c,m]              one kernel-row transform
 *                                                                 per (k, c, i), serving every b, as the forward
 * and after the last chunk grad_in[b,c,i,j] = IFFT_Pw(S[b,c,i,:])[j], j < W, unnormalised.  The planes
 * are summed in the spectrum: one inverse transform per input row, whatever Z.  VRS (Ez = Ex x/r_k +
 * Ey y/r_k carries the plane's z in r_k): output planes 0 / 1 as above; the third plane's product rows
 * are kept per plane of the chunk, inverted, multiplied by x_i / r_k and y_j / r_k and added to
 * grad_in[0] and grad_in[1] by the lane that owns the element, in plane order; the summed rows are
 * added last.  The first chunk stores S and the VRS terms (grad_in may be uninitialised memory; every
 * element is written), later chunks read, add and store on the same stream: no memset, no atomics, a
 * fixed summation order, so two calls with the same inputs are bit-identical; no transform along H,
 * no Ph x Pw table.  (W = 1: grad_out is empty and grad_in is set to zero, the one memset.)
 * Purely additive: THZ_ABI_VERSION stays 9, a caller detects the entries by symbol.  Validation is the
 * forward's, all before any device call: its shape rules; a bad row, Z outside 1 .. THZ_MAX_Z or a
 * null pointer THZ_E_ARG; a short or null workspace THZ_E_WORKSPACE (the message names the size).
 * Workspace:
 *   8 (vectorial ? 2 + zc : B) C H Pw      S, the summed spectra (VRS: Ex, Ey and the chunk's Ez product rows)
 * + 8 zc Bo C Pw                           Gh, one chunk's cotangent lines
 * bytes, each part rounded up to 256 -- no Ph x Pw table, no growth with Z past one chunk.
 */
int thz_rsc_slice_adjoint_workspace_size(const thz_rsc_slice_desc* d, size_t* bytes);
int thz_rsc_slice_adjoint(const thz_rsc_slice_desc* d, const void* grad_out /* [Z,Bo,C,Pw-W] */,
                          void* grad_in /* [B,C,H,W] */, void* workspace, size_t workspace_bytes,
                          thz_stream_t stream);

/* The Rayleigh-Sommerfeld kernel exp(i k r) z / (2 pi r^2) (1/r - i k), r = sqrt(x^2 + y^2 + z^2),
 * k = 2 pi / lambda_c, on n mesh points: CZT_prop.RS_kernel (Props/CZT_Prop.py:44-57) and the
 * spatial kernel of RSC_prop.create_kernel (Props/RSC_Prop.py:144-167).  x[n], y[n] device
 * floats (the meshes), wavelengths[C] host floats; out [C][n] complex64 (device). */
int thz_rs_kernel(const float* x, const float* y, int n, float z, const float* wavelengths, int C, void* out,
                  thz_stream_t stream);

/*
 * DOE modulation, DOELayer.modulate (Components/QuantizedDOE.py:92-126):
 *   h' = height + (noise - 0.5) * 2 * tolerance   (noise = the rand_like draw, NULL = no noise, :82-87)
 *   h_full = nearest-upsample(h') to [H, W]        (:102-107)
 *   out[b,c] = field[b,c] * exp(-k_c/2 (h+b) tand sqrt(eps)) exp(-i k_c (h+b)(sqrt(eps)-1))  (:47-79)
 * field/out [B, C, H, W] complex64; height/noise [hs, ws] float32 (device).  height_full, if
 * non-NULL, receives h_full [H, W].  Backward: grad_field = g conj(t) (NULL to skip) and
 * grad_height [hs, ws] = sum_bc Re(g conj(field) conj(dt/dh)) (NULL to skip).
 */
typedef struct thz_doe_desc {
  int B, C, H, W;
  int hs, ws;                /* height-map size (upsampled to H, W if different) */
  float tolerance, epsilon, tand;
  const float* wavelengths;  /* host [C] */
  const unsigned* rng;       /* optional DEVICE [2] = (seed, step): with noise == NULL the kernels draw
                                the U[0,1) height noise per height pixel from a counter-based generator
                                (hash of seed, step, rng_stream, index; forward and backward agree) */
  unsigned rng_stream;
} thz_doe_desc;

int thz_doe_modulate_forward(const thz_doe_desc* d, const void* field, const float* height, const float* noise,
                             void* out, float* height_full, thz_stream_t stream);
int thz_doe_modulate_backward(const thz_doe_desc* d, const void* grad_out, const void* field, const float* height,
                              const float* noise, void* grad_field, float* grad_height, thz_stream_t stream);

/*
 * Fused DOE -> ASM step: the ASM forward of thz_doe_modulate_forward(field) in one
 * pipeline -- the row pass applies the noisy, upsampled transmission t_c(h) in its loader, so the
 * modulated field never goes to memory.  Replaces DOELayer.modulate (Components/QuantizedDOE.py:
 * 92-126) followed by ASM_prop.forward (Props/ASM_Prop.py:314-378).  d: the ASM descriptor (forward,
 * adjoint == 0); m: the DOE descriptor of the same [B, C, H, W] field.  height_full (optional)
 * receives the noisy upsampled height map [H, W].  The backward composes the ASM adjoint and
 * thz_doe_modulate_backward.
 */
int thz_asm_forward_modulated(const thz_asm_desc* d, const thz_doe_desc* m, const void* field, const float* height,
                              const float* noise, float* height_full, void* out, void* workspace,
                              size_t workspace_bytes, thz_stream_t stream);

/*
 * Thick-element DOE: split-step (multi-slice) propagation through the relief.  The reference has no
 * counterpart (its thin screen leaves the field in the plane it entered); a slab's screen is
 * DOELayer.modulate's (Components/QuantizedDOE.py:47-126) on the slab's share of the height, a step is
 * ASM_prop.forward over dz (Props/ASM_Prop.py:314-378) with the descriptor's padding and band limit,
 * unpadded.  With dz = thickness / slices, z_s = s dz, d_s = clamp(h_full - z_s, 0, dz) (d_0 also
 * carries the base plate), h_full the nearest-upsampled map:
 *   t_{c,s} = exp(-k_c/2 d_s tand sqrt(eps)) exp(phase_sign i k_c d_s (sqrt(eps) - 1))
 *   U_{s+1} = ASM_dz(U_s t_s),  s = 0 .. slices-1;  out = U_slices, in the plane `thickness` above the base plate
 * phase_sign = -1 is DOELayer.modulate's sign (slices = 1 is then thz_asm_forward_modulated over
 * `thickness`), +1 the sign consistent with the ASM's exp(+i z k_z).  Heights above `thickness` count
 * as `thickness`, heights below 0 as 0; the map is never read back to the host.
 *   field / out [B, C, H, W] complex64, height [hs, ws] float32 (all device)
 * Two kernels per slab (a row pass that inverts, applies the next screen and transforms again in
 * LDS, and an in-place column pass) on one transfer-function table for every slab; the backward is
 * thz_thick_backward, below.
 * No allocation and no synchronisation per call (capturable in a HIP graph once the transform
 * lengths have been used).  Purely additive: THZ_ABI_VERSION stays 9, a caller detects the entries
 * by symbol.  Validation, all before any device call: a null pointer, a non-positive size,
 * thickness or slices, and |phase_sign| != 1 are THZ_E_ARG; padded sides H + 2 pad_h, W + 2 pad_w
 * other than powers of two from 64 to 8192 (they may differ), slices > 256 and C >
 * THZ_MAX_WAVELENGTHS are THZ_E_UNSUPPORTED; a short or null workspace THZ_E_WORKSPACE.
 * Workspace: the row spectra of the H window rows X [BC][H][Pw] and the table [C][Ph][Pw], complex64.
 */
typedef struct thz_thick_desc {
  int B, C, H, W, pad_h, pad_w, bandlimit, hs, ws, slices;
  float thickness, dx, dy, epsilon, tand, phase_sign;
  const float* wavelengths; /* host [C] */
} thz_thick_desc;
int thz_thick_workspace_size(const thz_thick_desc* d, size_t* bytes);
int thz_thick_forward(const thz_thick_desc* d, const void* field, const float* height, void* out, void* workspace,
                      size_t workspace_bytes, thz_stream_t stream);

/*
 * Thick-element DOE, native backward (additive: THZ_ABI_VERSION stays 9, detect by symbol).  The
 * reference has no counterpart; the pieces are DOELayer.modulate's screen and its derivative
 * (Components/QuantizedDOE.py:47-126, :73-77) and the adjoint of ASM_prop.forward (Props/ASM_Prop.py:314-378).
 *
 * One step is A = crop F^-1 diag(H_dz) F pad with the window at the origin of the padded plane, so
 * A^H = crop F^-1 diag(conj H_dz) F pad: the forward's passes with the table read conjugated.
 * d_s = clamp(h - z_s, 0, dz) moves with h only in the pixel's ACTIVE SLAB, where t_s' = kappa_c t_s,
 *   kappa_c = -(k_c/2) tand sqrt(eps) + phase_sign i k_c (sqrt(eps) - 1).
 * With V_s = U_s t_s and gU_S = grad_out:
 *   gV_s = A^H gU_{s+1},  gU_s = conj(t_s) gV_s  (s = S-1 .. 0),  grad_field = gU_0
 *   grad_height[r][c] = sum over b, c and the window pixels p whose nearest source is (r, c) of
 *                       Re(conj(kappa_c V_{s(p)}(p)) gV_{s(p)}(p)),  s(p) the active slab of p
 * Active-slab rule, the one definition the saving forward and the backward share: in fp32, with
 * z_s = (float)(s dz) and dz = (float)(thickness / slices) as the screens use them, slab s is active at a
 * pixel of height h when 0 < h - z_s < dz and slab s + 1 does not pass the same test (two neighbours can
 * pass only for h within an ulp of a face; the upper one then counts).  h - z_s is the very value the
 * screen clamps.  A height exactly on a face, on 0 or on `thickness`, below 0 or above `thickness` has no
 * active slab and a gradient of exactly 0; torch.clamp's inclusive rule differs on the faces only.
 *
 * thz_thick_forward_saved: thz_thick_forward (the same launches, `out` bit-identical) whose first and
 * middle row passes also store V_s at the pixels whose active slab is s into
 *   stash [B C][H][W] complex64 (device).  Pixels without an active slab keep what the buffer held: never read.
 * thz_thick_backward: grad_out [B, C, H, W] complex64, height as in the forward, stash from
 * thz_thick_forward_saved of the same descriptor, field and map.  grad_field [B, C, H, W] complex64 or NULL
 * (skipped); grad_height [hs, ws] float32 or NULL (no partials, no reduction; stash may then be NULL).
 * Launches: one row pass (grad_out rows, zero-padded, FFT), `slices` conjugate column passes, `slices` - 1
 * middle row passes (IFFT, the height partial where the slab is active, x conj(t_s), FFT), a closing row
 * pass (s = 0: partial and grad_field) and one reduction whose sums over b, c and the upsample footprint
 * are fp64 in a fixed order: the result is deterministic, and no atomics are used.
 * No allocation and no synchronisation per call; capturable on one stream.
 * Validation as thz_thick_forward, all before any device call: descriptor errors THZ_E_ARG, then
 * unsupported geometries THZ_E_UNSUPPORTED, then a null data pointer (grad_out, height, both gradients
 * NULL, grad_height without a stash) THZ_E_ARG, then a short or null workspace THZ_E_WORKSPACE.
 * Backward workspace: thz_thick_workspace_size + 4 B C H W (the partials, float32) rounded up to 256.
 */
int thz_thick_forward_saved(const thz_thick_desc* d, const void* field, const float* height, void* out, void* stash,
                            void* workspace, size_t workspace_bytes, thz_stream_t stream);
int thz_thick_backward_workspace_size(const thz_thick_desc* d, size_t* bytes);
int thz_thick_backward(const thz_thick_desc* d, const void* grad_out, const float* height, const void* stash,
                       void* grad_field, float* grad_height, void* workspace, size_t workspace_bytes,
                       thz_stream_t stream);

/*
 * Height-map quantizers of the QAT layers (forward value + custom backward), one fused kernel
 * each way.  weight: [hq, wq] (FP/STE/PSQ/SGV3) or [hq, wq, L] logits (NGS).  height_full:
 * [2hq, 2wq] when mirror (num_unit set, _copy_quad_to_full :28-35) else [hq, wq].
 * noise_exp: the Exp(1) draw F.gumbel_softmax consumes ([L, hq, wq] for SGV1 and for SGV3
 * when iter_frac > 0.3, [hq, wq, L] for NGS); y_soft (same shape) is saved for the backward.
 * SoftGumbelQuantizedDOELayerv2 (:608-635) is SGV3 with iter_frac passed as 0 or 1.
 */
#define THZ_Q_FP 0    /* FullPrecisionDOELayer            :286-292   */
#define THZ_Q_STE 1   /* STEQuantizedDOELayer             :1239-1388 */
#define THZ_Q_PSQ 2   /* PSQuantizedDOELayer              :1193-1223 */
#define THZ_Q_SGV3 3  /* SoftGumbelQuantizedDOELayerv3    :794-860   */
#define THZ_Q_NGS 4   /* NaiveGumbelQuantizedDOELayer     :1022-1041 */
#define THZ_Q_SGV1 5  /* SoftGumbelQuantizedDOELayer      :411-456 (weight = phase) */
#define THZ_MAX_LUT 16

typedef struct thz_quant_desc {
  int kind;
  int hq, wq;
  int mirror;
  int L;
  const float* lut;   /* host [L] */
  float hmax;         /* height_constraint_max */
  float clamp;        /* weight clamp: 8 (FP/STE/PSQ), 10 (SGV3) */
  float tau;          /* temperature of the layer's schedule */
  float iter_frac;    /* SGV3 schedule phase */
  float c_s;          /* SGV3 score boost */
  float s;            /* SGV3 steepness tau_max / tau */
  float beta;         /* SGV3 blend (iter_frac - 0.3) / 0.5 */
  float phase_scale;  /* SGV3 2 pi / lambda_min * (sqrt(eps) - 1), fp32 */
  const float* dyn;   /* optional DEVICE [3] = (tau, s, beta) read by the kernels instead of the
                         fields above, so one captured HIP graph serves every schedule step */
  const unsigned* rng; /* optional DEVICE [2] = (seed, step): with noise_exp == NULL the Gumbel
                          kinds draw their Exp(1) noise in the kernel (see thz_doe_desc.rng) */
  unsigned rng_stream;
} thz_quant_desc;

int thz_quant_forward(const thz_quant_desc* d, const float* weight, const float* noise_exp, float* height_full,
                      float* y_soft, thz_stream_t stream);
int thz_quant_backward(const thz_quant_desc* d, const float* weight, const float* y_soft, const float* grad_full,
                       float* grad_weight, thz_stream_t stream);

/*
 * The whole backward of a quantized DOE layer whose height map has the field's size (no nearest
 * upsampling): thz_doe_modulate_backward followed by thz_quant_backward in ONE kernel, the height
 * gradient never written (DOELayer.modulate :92-126 and the quantizer's backward, e.g. v3
 * :794-860).  d: the modulation (hs == H, ws == W); q: the quantizer that produced `height`
 * (its full map, mirrored or not, must be [H, W]).  grad_field (NULL to skip) as
 * thz_doe_modulate_backward, grad_weight as thz_quant_backward; bit-identical to the two calls.
 * THZ_E_UNSUPPORTED for an upsampled map (use the two calls).
 */
int thz_doe_quant_backward(const thz_doe_desc* d, const thz_quant_desc* q, const void* grad_out, const void* field,
                           const float* height, const float* noise, const float* weight, const float* y_soft,
                           void* grad_field, float* grad_weight, thz_stream_t stream);

/*
 * Radial profile -> 2-D height map of the rotationally symmetric layers
 * (Components/QuantizedDOE.py:1409-1433): quadrant pixel (x, y) takes profile[floor(r)] for
 * r = sqrt(x^2 + y^2) < R - 1 (0 beyond), mirrored to 2R x 2R and centre-cropped to [H, W].
 */
int thz_radial_forward(const float* profile, int R, int H, int W, float* out, thz_stream_t stream);
int thz_radial_backward(const float* grad_out, int R, int H, int W, float* grad_profile, thz_stream_t stream);
/* The rotationally symmetric layer's backward from the map gradient to its weight in one kernel:
 * thz_radial_backward then thz_quant_backward of the profile quantizer q (hq * wq == R, mirror 0;
 * weight / y_soft as thz_quant_backward), the profile gradient gathered per bin in a fixed order
 * (deterministic; thz_radial_backward scatters with atomics). */
int thz_radial_quant_backward(const thz_quant_desc* q, const float* grad_map, int R, int H, int W, const float* weight,
                              const float* y_soft, float* grad_weight, thz_stream_t stream);

/*
 * Optical elements around the DOE, generated / applied on the device.
 *
 * Guassian_beam.forward (LightSource/Gaussian_beam.py:88-160): out [1, C, H, W] complex64.
 * waist_x / waist_y: host [C] fp32 beam waists (given, or BeamWaistCorruagtedTK :67-85).
 */
typedef struct thz_gauss_desc {
  int C, H, W;
  float dx, dy;                /* field spacing */
  const float* wavelengths;    /* host [C] */
  const float* waist_x;        /* host [C] */
  const float* waist_y;        /* host [C] */
  float x0, y0;                /* beam centre */
  float z_w0x, z_w0y;          /* waist positions */
  float alpha;                 /* amplitude rotation (rad) */
} thz_gauss_desc;
int thz_gaussian_beam(const thz_gauss_desc* d, void* out, thz_stream_t stream);

/* Thin_LensElement.forward (Components/Thin_Lens.py:31-85): out = in * exp(-i pi r^2 / (lambda f)). */
typedef struct thz_lens_desc {
  int B, C, H, W;
  float dx, dy, focal_length;
  const float* wavelengths;    /* host [C] */
} thz_lens_desc;
int thz_thin_lens(const thz_lens_desc* d, const void* in, void* out, thz_stream_t stream);

/* ApertureElement.forward (Components/Aperture.py:44-136): out = in * mask (in == out allowed). */
#define THZ_APERTURE_RECT 1
#define THZ_APERTURE_CIRC 2
typedef struct thz_aperture_desc {
  int BC, H, W, kind;
  float dx, dy;
  float half_w, half_h;        /* rect: open where |x| <= half_w and |y| <= half_h (fp32) */
  float radius;                /* circ: open where sqrt(x^2 + y^2) <= radius */
} thz_aperture_desc;
int thz_aperture(const thz_aperture_desc* d, const void* in, void* out, thz_stream_t stream);

/*
 * QAT loss (experiment_four_focal_spots.ipynb:336-370): mean((normalize(|E|^2) - target)^2) with
 * normalize dividing each batch item by its max (utils/Helper_Functions.py:185-193).
 * target [tB, tC, H, W] broadcast over B / C (tB in {1, B}, tC in {1, C}).
 * stats: device workspace of thz_intensity_mse_workspace_size bytes (max, argmax, max-path sum
 * per batch item, kept for the backward); loss: device [1]; grad_loss: device [1].
 */
typedef struct thz_loss_desc {
  int B, C, H, W;
  int tB, tC;
} thz_loss_desc;
size_t thz_intensity_mse_workspace_size(const thz_loss_desc* d);
int thz_intensity_mse_forward(const thz_loss_desc* d, const void* field, const float* target, float* loss,
                              float* stats, thz_stream_t stream);
int thz_intensity_mse_backward(const thz_loss_desc* d, const void* field, const float* target, const float* stats,
                               const float* grad_loss, void* grad_field, thz_stream_t stream);

/*
 * Fused ASM -> loss step: ASM forward of one z-plane (optionally of the DOE
 * modulation of field, as thz_asm_forward_modulated; m == NULL: plain ASM, height / noise /
 * height_full ignored) whose row-inverse pass also accumulates the QAT loss above over the rows
 * it stores, so the output field is not read back.  Replaces ASM_prop.forward (Props/
 * ASM_Prop.py:314-378) followed by the notebook's loss (experiment_four_focal_spots.ipynb:
 * 336-370, normalize = utils/Helper_Functions.py:185-193).  l describes the ASM output
 * [B, C, Ho, Wo]; out, loss and stats are what thz_asm_forward and thz_intensity_mse_forward
 * return (stats: thz_intensity_mse_workspace_size bytes, valid for thz_intensity_mse_backward).
 * Z > 1 planes (the multi-plane notebooks, e.g. plot_data/example_2 / example_3): l describes the
 * Z x B plane-major items [Z B, C, Ho, Wo] (each normalised by its own max; target tB in {1, Z B})
 * and the loss is the SUM over the planes of each plane's mean -- the notebooks' summed MSEs.
 */
/*
 * Its backward's first half in one pipeline: the ASM adjoint (d->adjoint == 1; Z >= 1 with l as above,
 * the Z-summing adjoint) of the loss
 * gradient dL/dE = 2 E dL/dI at the forward output `field` (thz_intensity_mse_backward's formula,
 * from the same target, stats and device grad_loss [1]), plus grad_out when non-NULL (the
 * cotangent of the output field itself).  The row pass forms the gradient as it loads each row.
 */
int thz_asm_adjoint_loss(const thz_asm_desc* d, const thz_loss_desc* l, const void* field, const float* target,
                         const float* stats, const float* grad_loss, const void* grad_out, void* grad_in,
                         void* workspace, size_t workspace_bytes, thz_stream_t stream);
int thz_asm_forward_loss(const thz_asm_desc* d, const thz_doe_desc* m, const void* field, const float* height,
                         const float* noise, float* height_full, const thz_loss_desc* l, const float* target,
                         void* out, float* loss, float* stats, void* workspace, size_t workspace_bytes,
                         thz_stream_t stream);

/*
 * Field_Resampler.forward (Addons/Field_Resampler.py:74-118): bilinear grid_sample (zeros
 * padding, align_corners=True) of [BC, Hin, Win] complex64 onto the centred output grid
 * linspace(-((n-1)//2), (n-1)//2, n) * d_out, normalised by d_in * ((n_in - 1) // 2).
 * The backward scatters grad_out with the same weights (grad_in is zeroed first).
 */
typedef struct thz_resample_desc {
  int BC, Hin, Win, Hout, Wout;
  float dx_in, dy_in, dx_out, dy_out;
} thz_resample_desc;
int thz_resample_forward(const thz_resample_desc* d, const void* in, void* out, thz_stream_t stream);
int thz_resample_backward(const thz_resample_desc* d, const void* grad_out, void* grad_in, thz_stream_t stream);

/*
 * Polarization analysis of a vectorial field (Addons/Polarization.py:45-92,
 * PolarizationAnalyser.polarization_state / polarization_ellipse), one streaming pass each.
 * ex, ey: the Ex and Ey component planes, each n contiguous complex64 values (8-byte aligned; the
 * planes of a [B >= 2, ...] tensor -- the Ez plane is never passed or read).  Outputs are four
 * planes of n floats, [4][n] contiguous.  Null pointers and n < 0 are THZ_E_ARG; n == 0 is THZ_OK
 * and launches nothing.  When every pointer is 16-byte aligned and n % 4 == 0 each lane moves its
 * four pixels as 16-byte accesses; otherwise the same kernel body runs with element-width accesses
 * (bit-identical results).
 *
 * thz_stokes_forward (:49-56): out = I, Q, U, V with
 *   I = |Ex|^2 + |Ey|^2,  Q = |Ex|^2 - |Ey|^2,  U = 2 Re(Ex conj Ey),  V = 2 Im(Ex conj Ey).
 * thz_stokes_backward: the cotangent of a real loss in torch's convention (dL/dRe + i dL/dIm),
 * grad = gI, gQ, gU, gV [4][n]:
 *   gEx = 2 [(gI + gQ) Ex + (gU + i gV) Ey],   gEy = 2 [(gI - gQ) Ey + (gU - i gV) Ex].
 * thz_polarization_ellipse (:72-84): out = A, B, theta, h from the fields in one pass (the Stokes
 * planes are not materialised), the reference's sequence in its order with eps = 1e-6:
 *   Ip = sqrt(Q^2 + U^2 + V^2),  L = (Q + eps) + i U,
 *   A = sqrt((Ip + |L| + eps) / 2),  B = sqrt((Ip - |L| + eps) / 2),
 *   theta = atan2(U, Q + eps) / 2,  h = sign(V + eps).
 * One deliberate deviation: for exactly linear polarization rounding can leave B's radicand
 * slightly negative, where the reference returns NaN; the radicand is clamped at 0 here.
 */
int thz_stokes_forward(const void* ex, const void* ey, long long n, float* out, thz_stream_t stream);
int thz_stokes_backward(const void* ex, const void* ey, long long n, const float* grad, void* gex, void* gey,
                        thz_stream_t stream);
int thz_polarization_ellipse(const void* ex, const void* ey, long long n, float* out, thz_stream_t stream);

/*
 * Detector noise models (Addons/Noise.py:4-112, utils/Noise.py:4-116, utils/Helper_Functions.py:
 * 258-366: GaussianNoise, PoissonNoise, PoissonGaussianNoise, UniformNoise) on the counter-based
 * device generator of thz_doe_desc.rng: every draw is a hash of (seed, step, stream, element
 * index), so a call is reproducible from its state, independent of the launch geometry, and a
 * captured graph draws afresh on every replay once its host advances rng[1].  No torch RNG kernel
 * and no host synchronisation anywhere.  fp32 / complex64 only.
 *
 * thz_noise_apply: one streaming pass, out[i] = model(in[i]) for i < n, fp32 in the reference's
 * operation order (x is in[i], or |in[i]|^2 = abs() ** 2 for THZ_NOISE_IN_FIELD_INTENSITY):
 *   THZ_NOISE_GAUSS          x + n sigma                              (Addons/Noise.py:27)
 *   THZ_NOISE_UNIFORM        x + (u - 0.5) 2 a                        (:112)
 *   THZ_NOISE_POISSON        poisson(x / gain), then * gain if normalize   (:58-61)
 *   THZ_NOISE_POISSON_GAUSS  poisson(x / gain) gain + n sigma         (:87-89)
 * n is a standard normal (Box-Muller on two 24-bit uniforms, |n| <= 5.77), u is U[0, 1) with 24
 * bits, both drawn at (stream, i); the Poisson draw of element i reads a 64-bit sequence of its
 * own, seeded by a hash of (stream, i) and advanced per attempt, that its n never touches and
 * that two streams do not share (inversion below a rate of 10, transformed rejection PTRS from
 * 10; rates up to 2^24, where fp32 still holds every count; a rate of 0 gives 0, a negative or
 * NaN rate gives NaN -- no host check, that would be a sync).  Streams are independent under one
 * seed: the generator mixes the stream into the seed word (seed ^ stream * 0x9E3779B9), so two
 * (seed, stream) pairs with the same mix draw the same values.  THZ_NOISE_IN_COMPLEX64 (GAUSS only): in and out are complex64 and n is a complex
 * normal of total variance 1 (torch.randn_like of a complex tensor), both Box-Muller outputs of
 * the element's word.  sigma_dev, when not NULL, is a device scalar read in place of sigma (the
 * SNR form, utils/Noise.py:28-32, with thz_signal_scale's output).
 * in: n floats (REAL32) or n complex64 (FIELD_INTENSITY, COMPLEX64); out: n floats, or n
 * complex64 for COMPLEX64; in and out do not overlap.  When both
 * pointers are 16-byte aligned and n % 4 == 0 a lane moves four elements per 16-byte access;
 * otherwise the same body runs at element width (bit-identical results).
 * Null pointers (d, in, out, d->rng), n < 0, n > 2^32 (the generator's index is 32-bit), an unknown
 * kind or input, COMPLEX64 with a kind other than GAUSS and gain <= 0 for the Poisson kinds are
 * THZ_E_ARG; n == 0 is THZ_OK and launches nothing.
 */
#define THZ_NOISE_GAUSS 0
#define THZ_NOISE_UNIFORM 1
#define THZ_NOISE_POISSON 2
#define THZ_NOISE_POISSON_GAUSS 3
#define THZ_NOISE_IN_REAL32 0
#define THZ_NOISE_IN_FIELD_INTENSITY 1
#define THZ_NOISE_IN_COMPLEX64 2
typedef struct thz_noise_desc {
  int kind;                /* THZ_NOISE_* */
  int input;               /* THZ_NOISE_IN_* */
  float sigma, a, gain;
  int normalize;           /* POISSON: multiply the counts by gain */
  const float* sigma_dev;  /* device [1] or NULL: replaces sigma */
  const unsigned* rng;     /* device [2] = {seed, step} */
  unsigned stream;
} thz_noise_desc;
int thz_noise_apply(const thz_noise_desc* d, const void* in, void* out, long long n, thz_stream_t stream);

/*
 * The raw draws thz_noise_apply uses for elements 0 .. n-1 of (rng, stream), so a caller can hold
 * the kernels to the reference's formulas exactly: THZ_DRAW_NORMAL out[n] = n_i, THZ_DRAW_UNIFORM
 * out[n] = u_i, THZ_DRAW_COMPLEX_NORMAL out[2 n] = (Re, Im) of the complex normal, interleaved.
 * Validation as thz_noise_apply.
 */
#define THZ_DRAW_NORMAL 0
#define THZ_DRAW_UNIFORM 1
#define THZ_DRAW_COMPLEX_NORMAL 2
int thz_noise_draws(int what, const unsigned* rng, unsigned stream, long long n, float* out, thz_stream_t stream_handle);

/*
 * The noise amplitude of the SNR form of GaussianNoise (utils/Noise.py:28-32):
 *   scale[0] = sqrt(mean(|x|^2) / snr_linear),  snr_linear = 10 ** (SNR_dB / 10),
 * x: n floats (is_complex == 0) or n complex64, scale: a device scalar (feed it to
 * thz_noise_desc.sigma_dev).  Summed in fp64 and rounded to fp32 once, in two stages: one partial
 * per workgroup in the workspace (a grid that depends on n alone), then one workgroup adds the
 * partials in a fixed order -- the same input always gives the same bits.  No host sync.
 * Null pointers, n < 0, n > 2^32 and snr_linear <= 0 are THZ_E_ARG; a workspace below
 * thz_signal_scale_workspace_size(n) is THZ_E_WORKSPACE; n == 0 is THZ_OK and launches nothing.
 *
 * thz_snr_noise_backward: the cotangent of y = x + n scale(x) (torch's convention for complex x),
 * the noise regenerated from (rng, stream):
 *   gx = g + x S / (N snr_linear scale),  S = sum_i Re(conj(g_i) n_i),
 * S reduced in fp64 as above.  g, x and gx have x's element type; scale is thz_signal_scale's
 * output for this x; same workspace size.
 */
int thz_signal_scale_workspace_size(long long n, size_t* bytes);
int thz_signal_scale(const void* x, long long n, int is_complex, float snr_linear, float* scale, void* workspace,
                     size_t bytes, thz_stream_t stream);
int thz_snr_noise_backward(const void* g, const void* x, long long n, int is_complex, float snr_linear,
                           const float* scale, const unsigned* rng, unsigned stream, void* gx, void* workspace,
                           size_t bytes, thz_stream_t stream_handle);

/*
 * The image losses of utils/losses.py on contiguous float32 device arrays (thz_losses.hip).
 *
 * Dice and BCE (BinaryDiceLoss utils/losses.py:21-44, BinaryCEloss utils/losses.py:48-58) share one
 * streaming pass over pred, target viewed as [N, M].  thz_dice_bce_sums writes sums[N][4] (double):
 *   sum p t,  sum p^e,  sum t^e  (utils/losses.py:32-33; e = p of the descriptor, 1 and 2 without powf)
 *   sum bce(p, t),  bce = max(x, 0) - x t + log1p(exp(-|x|))  (torch.nn.BCEWithLogitsLoss, utils/losses.py:54);
 * with weight / pos_weight (device [N M], either may be NULL) torch's
 *   ((1 - t) x + (1 + (pos_weight - 1) t) (log1p(exp(-|x|)) + max(-x, 0))) weight.
 * terms selects what is formed (a sum that is not is 0); bce_map (device [N M] or NULL) also receives
 * the elementwise BCE (reduction='none').  fp64 partial per workgroup in the workspace, on a grid
 * that depends on (N, M) alone, then a finish kernel adds the partials in index order: no atomics,
 * the same input gives the same bits, aligned or not.  16-byte accesses when every pointer is
 * 16-byte aligned and M % 4 == 0, the same body at element width otherwise.
 *
 * thz_dice_bce_backward writes grad_pred [N M] in one pass from the saved sums and the upstream
 * gradients, which stay on the device (no host sync):
 *   DICE: g_dice[n] d/dp (1 - num / den) = -g_dice[n] (t den - num e p^(e-1)) / den^2,
 *         num = sum p t + smooth, den = sum p^e + sum t^e + smooth  (utils/losses.py:32-35)
 *   BCE:  g_bce (sigma(x) - t), weighted  g_bce weight ((1 - t) - (1 + (pos_weight - 1) t) (1 - sigma(x)));
 *         g_bce is a device scalar, or [N M] when bce_grad_elementwise (reduction='none').
 * Both terms in one pass when terms has both (Hierarchyloss, utils/losses.py:86-88).
 * A null descriptor or pointer, N < 1, M < 1 and terms outside DICE | BCE are THZ_E_ARG; N > 2^24 is
 * THZ_E_UNSUPPORTED; a workspace below thz_dice_bce_sums_workspace_size is THZ_E_WORKSPACE.
 */
#define THZ_LOSS_TERM_DICE 1
#define THZ_LOSS_TERM_BCE 2
typedef struct thz_dice_bce_desc {
  long long N, M;
  float p;                   /* the Dice exponent (utils/losses.py:21: 2) */
  float smooth;              /* utils/losses.py:21: 1 (backward only; the sums carry no smooth) */
  int terms;                 /* THZ_LOSS_TERM_DICE | THZ_LOSS_TERM_BCE */
  int bce_grad_elementwise;  /* backward: g_bce is [N M] */
  const float* weight;       /* device [N M] or NULL */
  const float* pos_weight;   /* device [N M] or NULL */
} thz_dice_bce_desc;
int thz_dice_bce_sums_workspace_size(const thz_dice_bce_desc* d, size_t* bytes);
int thz_dice_bce_sums(const thz_dice_bce_desc* d, const float* pred, const float* target, double* sums,
                      float* bce_map, void* workspace, size_t bytes, thz_stream_t stream);
int thz_dice_bce_backward(const thz_dice_bce_desc* d, const float* pred, const float* target, const double* sums,
                          const float* g_dice, const float* g_bce, float* grad_pred, thz_stream_t stream);

/*
 * SSIM (SSIMloss utils/losses.py:62-74, which wraps pytorch_msssim.SSIM) of x, y [NC][H][W]: the
 * mean over the window positions [H - ws + 1][W - ws + 1] of
 *   S = A1 A2 / (B1 B2),  A1 = 2 mu_x mu_y + C1,  A2 = 2 sigma_xy + C2,
 *   B1 = mu_x^2 + mu_y^2 + C1,  B2 = sigma_x^2 + sigma_y^2 + C2,
 *   sigma_x^2 = m_xx - mu_x^2,  sigma_xy = m_xy - mu_x mu_y,  C1 = (K1 L)^2,  C2 = (K2 L)^2,
 * mu, m the separable window's means of x, y, x^2, y^2, xy.  window: the ws taps of the 1-D window,
 * formed by the caller (pytorch_msssim: exp(-(i - ws / 2)^2 / (2 sigma^2)) normalised in fp32); ws odd,
 * 1 .. THZ_SSIM_MAX_WIN, anything else THZ_E_UNSUPPORTED.  The kernels filter in fp64 with the taps
 * divided by their own fp64 sum: fp32-normalised taps sum to 1 + delta (|delta| ~ 1e-8), which exact
 * arithmetic would turn into a variance of -delta x^2 on a flat region, amplified by 1 / C2 into S;
 * fp32 arithmetic never resolves delta and the definition has none.  An axis shorter than ws is not filtered
 * (one tap of 1 on it), as pytorch_msssim does.  One workgroup per 32 x 32 tile of positions stages
 * its tiles of x and y in LDS once and filters in fp64; ssim[NC] (relu'd when nonnegative) and cs[NC]
 * (the mean of A2 / B2; may be NULL) come from fp64 partials per workgroup added in index order.
 * coef (device [3][NC][H'][W'] or NULL) receives a = dS/dmu_x, b = dS/dm_xx, c = dS/dm_xy:
 *   c = 2 A1 / (B1 B2),  b = -S / B2,  a = 2 mu_y (A2 - A1) / (B1 B2) - 2 mu_x S (1 / B1 - 1 / B2).
 *
 * thz_ssim_backward: grad_x[p] (+)= gate g[nc] / (H' W') ((w * a)[p] + 2 x[p] (w * b)[p] + y[p] (w * c)[p]),
 * * the full separable correlation over the positions whose window covers pixel p, gathered per
 * pixel (no atomics); g device [NC], the gradient of ssim[nc]; gate = (ssim[nc] > 0) when
 * nonnegative, else 1; accumulate adds into grad_x.
 * A null descriptor or pointer and NC, H or W < 1 are THZ_E_ARG; NC > 65535 is THZ_E_UNSUPPORTED.
 */
#define THZ_SSIM_MAX_WIN 33
typedef struct thz_ssim_desc {
  int NC, H, W;
  int ws;                          /* taps */
  float window[THZ_SSIM_MAX_WIN];  /* the first ws entries */
  double C1, C2;
  int nonnegative;                 /* nonnegative_ssim */
  int accumulate;                  /* backward: grad_x += */
} thz_ssim_desc;
int thz_ssim_workspace_size(const thz_ssim_desc* d, size_t* bytes);
int thz_ssim_forward(const thz_ssim_desc* d, const float* x, const float* y, float* ssim, float* cs, float* coef,
                     void* workspace, size_t bytes, thz_stream_t stream);
int thz_ssim_backward(const thz_ssim_desc* d, const float* x, const float* y, const float* coef, const float* ssim,
                      const float* g, float* grad_x, thz_stream_t stream);

/*
 * Look-up-table quantizers of a height map (thz_heightmap.hip).  x [n] float32; q [n] float32 = lut[idx];
 * idx [n] int32.  The L levels (1 .. THZ_MAX_LUT) and the T thresholds travel by value in the descriptor and
 * are compared in fp32 exactly as given, so q and idx equal torch's bit for bit.
 *   THZ_LUTQ_BUCKETIZE  nearest_idx / nearest_neighbor_search (utils/Helper_Functions.py:375-398):
 *       idx = #{j < T : !(thresholds[j] > x)} = torch.bucketize(x, thresholds, right=True) on ascending
 *       thresholds (a NaN x counts every threshold, as torch does); wrap != 0 then takes idx mod T -- the
 *       reference's `idx % len(lut_midvals)` (:398), which sends every x at or above the top threshold to
 *       level 0 (kept: a height map's top level is the phase wrap of level 0).  T <= L - 1 without wrap,
 *       1 <= T <= L with it, so idx < L.
 *   THZ_LUTQ_ARGMIN     the notebooks' quantization(input, lut) (experiment_extend_depth_of_focus.ipynb cell
 *       "def quantization", experiment_dual_plane_hologram.ipynb): idx = argmin_j |x - lut[j]|, the first
 *       minimum (ties to the lower index, as torch.argmin); a NaN x gives 0.  T is ignored.
 * One streaming pass, 4 B read and 8 B written per element; 16-byte accesses when x, q and idx are 16-byte
 * aligned (a last group that crosses n moves element by element), element-width accesses otherwise.
 *
 * thz_lut_quantize_backward: grad_in = grad_out f(x, idx) in one pass (16 B per element), the surrogate
 * gradients of Components/quantization.py:
 *   THZ_LUTQ_GRAD_IDENTITY  f = 1                                      (NearestNeighborSearch, :70-71)
 *   THZ_LUTQ_GRAD_POLY      f = nan_to_num(0.5 s (1 - |z|)^(s - 1)) 2  (NearestNeighborPolyGrad, :79-96)
 *   THZ_LUTQ_GRAD_SIGMOID   f = sigma(s z) (1 - sigma(s z)) 4 s        (NearestNeighborSigmoidGrad, :104-122)
 * with q = lut[idx], d = sign(x - q) (0 when x == q or x - q is not finite), other = lut[idx + d],
 * mid = (other + q) / 2, gap = |other - q| + 1e-20, z = 2 (x - mid) / gap; so x == q gives z = 0.  idx + d = -1
 * reads the last level, as the reference's negative index does; idx + d = L, where the reference's index
 * raises, reads level 0; a stored idx outside [0, L) is clamped into it.  s: device float [1], read by the
 * kernel (a captured graph sees each replay's value); NULL for the identity kind.
 * A null descriptor or pointer, n < 0, a mode or kind outside the lists and T outside the ranges above are
 * THZ_E_ARG; L outside 1 .. THZ_MAX_LUT is THZ_E_UNSUPPORTED.
 */
#define THZ_LUTQ_BUCKETIZE 0
#define THZ_LUTQ_ARGMIN 1
#define THZ_LUTQ_GRAD_IDENTITY 0
#define THZ_LUTQ_GRAD_POLY 1
#define THZ_LUTQ_GRAD_SIGMOID 2
typedef struct thz_lut_quantize_desc {
  long long n;
  int mode;                       /* THZ_LUTQ_BUCKETIZE / THZ_LUTQ_ARGMIN (forward) */
  int wrap;                       /* bucketize: idx mod T */
  int kind;                       /* THZ_LUTQ_GRAD_* (backward) */
  int L, T;                       /* levels, thresholds */
  float lut[THZ_MAX_LUT];
  float thresholds[THZ_MAX_LUT];
} thz_lut_quantize_desc;
int thz_lut_quantize_forward(const thz_lut_quantize_desc* d, const float* x, float* q, int* idx, thz_stream_t stream);
int thz_lut_quantize_backward(const thz_lut_quantize_desc* d, const float* x, const int* idx, const float* grad_out,
                              const float* s, float* grad_in, thz_stream_t stream);

/*
 * Total variation of a height map (utils/Helper_Functions.py:40-70) on x [N][H][W] float32 (the caller
 * flattens the leading dimensions).  center_difference (:56-70):
 *   dx[i][j] = W / 4 (-x[i][j-1] + 2 x[i][j] - x[i][j+1])  for 1 <= j <= W - 2, else 0
 *   dy[i][j] = H / 4 (-x[i-1][j] + 2 x[i][j] - x[i+1][j])  for 1 <= i <= H - 2, else 0
 * and total_variation (:40-54) = mean |dx| + mean |dy| over all N H W elements, borders included.
 * thz_tv_forward reads x once: a wave owns a tile of 256 columns x 32 rows, a lane four consecutive
 * columns; it walks down the rows with the previous, current and next row in registers and takes the
 * columns left and right of its four from the neighbouring lanes (the tile's own edge columns by a
 * one-element load).  With dx and dy non-NULL it writes both maps (tv, workspace may be NULL); with both
 * NULL it forms sum |dx| and sum |dy| as fp64 partials per workgroup in the workspace, added in index
 * order by a finish kernel that writes tv [1] -- no atomics, the same input gives the same bits.
 *
 * thz_tv_backward gathers the adjoint stencil per element (no atomics):
 *   grad[i][j] = W / 4 (2 u[i][j] - u[i][j-1] - u[i][j+1]) + H / 4 (2 v[i][j] - v[i-1][j] - v[i+1][j]),
 * u, v zero outside the interior columns / rows.  With x non-NULL (total_variation): u = sign(dx) g / (N H W),
 * v = sign(dy) g / (N H W), g = *grad_loss (device [1]), sign(0) = 0 as torch's abs backward; gdx, gdy NULL.
 * With x NULL (center_difference): u = gdx, v = gdy, the cotangents of the two maps; grad_loss NULL.
 * A null pointer and N, H or W < 1 are THZ_E_ARG; H or W above 2^30 and more than 2^31 - 1 workgroups are
 * THZ_E_UNSUPPORTED; a workspace below thz_tv_workspace_size is THZ_E_WORKSPACE.
 */
int thz_tv_workspace_size(long long N, int H, int W, size_t* bytes);
int thz_tv_forward(const float* x, long long N, int H, int W, float* dx, float* dy, float* tv, void* workspace,
                   size_t bytes, thz_stream_t stream);
int thz_tv_backward(const float* x, const float* gdx, const float* gdy, const float* grad_loss, long long N, int H,
                    int W, float* grad, thz_stream_t stream);

/*
 * Focal-spot figures of merit (thz_metrics.hip; quantizationawarethzdoe_amd/utils/metrics.py -- the
 * reference's utils/metrics.py is an empty placeholder, these follow its notebooks' conventions).
 *
 * thz_region_stats_forward: x is N contiguous planes of H x W elements of `dtype`: a field (complex64 /
 * complex128, interleaved re, im; I = re^2 + im^2 formed in fp64 with separate multiplies and one add) or an
 * intensity (float32 / float64, I = x).  regions: K (0 .. THZ_MAX_REGIONS) entries {kind, cr, cc, a, b} in
 * pixel units (row i, column j), a host table copied into the launch or, with regions_on_device, a device
 * table read by the kernels (then a kind other than THZ_REGION_CIRC is read as THZ_REGION_RECT):
 *   THZ_REGION_CIRC  (i - cr)^2 + (j - cc)^2 <= a^2        THZ_REGION_RECT  |i - cr| <= a and |j - cc| <= b
 * evaluated in fp64 from the fp32 values.  Region index K is the whole plane.
 * out: fp64 [N, K + 1, 8] = S0 = sum I, Sr = sum I i, Sc = sum I j, Srr = sum I i^2, Scc = sum I j^2,
 * peak = max I, argmax (the lowest flat index i W + j that attains it), count (pixels inside).  A region with
 * no pixel in the plane gives zeros, peak = 0 and argmax = -1; a NaN never wins the peak.
 * One pass: an element is read once for all regions (a 256 x 32 tile visits only the regions whose bounding
 * box meets it); fp64 sums per workgroup in a fixed order into the workspace, merged per plane in tile order by
 * a second launch -- no atomics, the same input gives the same bits; no host read.  16-byte loads when x is
 * 16-byte aligned and a row's bytes are a multiple of 16, element-width loads otherwise (same results).
 *
 * thz_region_stats_backward: G fp64 [N, K + 1, 5], the cotangents of the five sums; one pass writes
 *   grad_I(n, i, j) = sum over the regions k holding (i, j) of G0 + G1 i + G2 j + G3 i^2 + G4 j^2
 * as grad_I (intensities; x may be NULL) or 2 grad_I x (fields, the convention of thz_stokes_backward) in
 * x's dtype.  peak, argmax and count carry no gradient.
 *
 * thz_line_widths: v is L contiguous lines of W samples (THZ_METRICS_F32 / THZ_METRICS_F64), 0 < level < 1.
 * out: fp64 [L, 5] = peak, argmax (lowest index), xl, xr, xr - xl, the nearest crossings of t = level peak on
 * either side of the peak, in samples: with j the largest index below argmax with v[j] < t,
 * xl = j + (t - v[j]) / (v[j + 1] - v[j]) in fp64; xr the mirror image, j the smallest index above argmax with
 * v[j] < t, xr = j - (t - v[j]) / (v[j - 1] - v[j]).  A side with no such sample gives NaN there and for the
 * width.  A wave per line up to 1024 samples, a workgroup per line beyond.
 *
 * A null descriptor / pointer, negative N, H, W or L, W < 1 (lines), K outside 0 .. THZ_MAX_REGIONS, an unknown
 * dtype or host region kind, a level outside (0, 1) and a misaligned array or workspace are THZ_E_ARG; H or W
 * above 2^30 and more than 2^31 - 1 workgroups are THZ_E_UNSUPPORTED; a workspace below
 * thz_region_stats_workspace_size is THZ_E_WORKSPACE.
 */
#define THZ_MAX_REGIONS 16
#define THZ_REGION_CIRC 0
#define THZ_REGION_RECT 1
#define THZ_METRICS_C64 0
#define THZ_METRICS_C128 1
#define THZ_METRICS_F32 2
#define THZ_METRICS_F64 3
typedef struct thz_region {
  int kind;          /* THZ_REGION_* */
  float cr, cc;      /* centre: row, column */
  float a, b;        /* circ: radius a (b unused); rect: half-height a, half-width b */
} thz_region;
typedef struct thz_region_stats_desc {
  long long N;               /* planes */
  int H, W;
  int dtype;                 /* THZ_METRICS_* */
  int K;                     /* 0 .. THZ_MAX_REGIONS */
  const thz_region* regions; /* [K]; NULL when K == 0 */
  int regions_on_device;     /* 0: host table, 1: device table */
} thz_region_stats_desc;
int thz_region_stats_workspace_size(const thz_region_stats_desc* d, size_t* bytes);
int thz_region_stats_forward(const thz_region_stats_desc* d, const void* x, double* out, void* workspace, size_t bytes,
                             thz_stream_t stream);
int thz_region_stats_backward(const thz_region_stats_desc* d, const void* x, const double* G, void* grad,
                              thz_stream_t stream);
int thz_line_widths(const void* v, int dtype, long long L, int W, double level, double* out, thz_stream_t stream);

/*
 * The projections of the iterative Fourier-transform algorithm (thz_ifta.hip; quantizationawarethzdoe_amd/
 * ifta.py -- the reference has no such designer): between the fused DOE -> ASM forward and the Z-summing ASM
 * adjoint, one iteration imposes the target amplitude on the planes and the level table on the height map.
 * U is N contiguous planes of H x W complex64 (interleaved re, im).  T is the target amplitude, float32, one
 * plane [H, W] for every plane of U (target_planes = 1) or [N, H, W] (target_planes = N), non-negative.  M is
 * the signal window, uint8 [H, W], non-zero inside; NULL: every pixel.  |U| = sqrt(re^2 + im^2) in fp64.
 *
 * thz_ifta_target_stats: one pass that reads U, T and M once.  out: fp64 [N, 6] =
 *   S_all = sum |U|^2, S_in = sum_M |U|^2, S_TU = sum_M T |U|, S_TT = sum_M T^2,
 *   s = S_TU / S_TT (0 when S_TT = 0), eff = S_in / S_all (0 when S_all = 0);
 * s is the least-squares scale of s T against |U| over M.  fp64 sums per workgroup (4096 pixels) in a fixed
 * order into the workspace, added per plane in index order by a second launch -- no atomics, the same input
 * gives the same bits; no host read.  out is any 8-byte aligned device address (a row of a history array).
 *
 * thz_ifta_target_project: out [N, H, W] complex64; scale: device fp64 [N], read by the kernel.
 *   inside M:   a' = max(0, alpha scale[n] T + (1 - alpha) |U|), out = a' U / |U|; where |U| = 0, out = a'
 *   outside M:  out = beta U
 * alpha = 1 is Gerchberg-Saxton, 1 < alpha <= 2 the over-compensated (adaptive-additive) form; beta = 1 leaves
 * the amplitude outside the window free, beta = 0 suppresses it.  Each pixel is formed in fp64 and rounded to
 * float32 once.  out == U (in place) is legal; any other overlap is not.
 * Both read and write 16 bytes per access when U, T and out are 16-byte aligned, M is 4-byte aligned and, with
 * more than one plane of U or T, H W is a multiple of 4; a last group that crosses the plane's end and every
 * other case move element by element (same results).  12 - 13 B read per pixel (stats), 13 B read and 8 B
 * written (project).
 *
 * thz_ifta_doe_project: the DOE has hs x ws cells of r_h x r_w field pixels each, H = r_h hs and W = r_w ws
 * (for these the nearest upsampling of the modulate kernels is block replication).  U [N, H, W] is the
 * back-propagated field; A the incident field, complex64 [H, W] (incident_planes = 1) or [N, H, W]
 * (incident_planes = N), or NULL with incident_planes = 0 for A = 1.  Per cell
 *   g = sum over the cell of U conj(A): products and sum in fp64, the cell's pixels in row-major order (the
 *       adjoint of the nearest upsampling);  phi = atan2(Im g, Re g), 0 for g = 0;
 *   the transmission phase of a height h is -kappa (h + base plane), kappa = 2 pi / lambda (sqrt(eps) - 1)
 *   formed in fp32 as the modulate kernels form it, so
 *   h_c = ((-phi) / kappa - base plane) mod h_max,  h_max = 2 pi / kappa;
 *   the nearest level on the circle of circumference h_max, the lowest index on a tie; d the cyclic distance
 *   to it and G half the gap to its neighbour on h_c's side (G = h_max / 2 for a single level);
 *   the cell takes the level when d <= q G or q >= 1, and keeps h_c otherwise.
 * q: device float [1], read by the kernel (a captured graph sees each replay's value); q = 0 leaves the map
 * continuous, q = 1 snaps every cell.  h: float32 [N, hs, ws], lut[idx] bit for bit where snapped; idx: int32,
 * the level or -1.  lut: L (1 .. THZ_MAX_LUT) levels ascending in [0, h_max), by value.  The loss tangent takes
 * no part: the projection fits the phase of the transmission alone, its amplitude exp(-k/2 (h + base) tand
 * sqrt(eps)) is neither compensated nor used as a weight.  8 - 16 B read per pixel, 8 B written per cell.
 *
 * All three are capturable and check their arguments before any device call: a null descriptor or pointer, a
 * misaligned array, a negative size, target_planes outside {1, N}, incident_planes outside {0, 1, N}, L outside
 * 1 .. THZ_MAX_LUT, a table that does not ascend or leaves [0, h_max), wavelength <= 0 or epsilon <= 1, alpha
 * outside (0, 2] and beta outside [0, 1] are THZ_E_ARG; a field that is not a whole number of pixels per cell
 * and more than 2^31 - 1 workgroups are THZ_E_UNSUPPORTED; a workspace below
 * thz_ifta_target_stats_workspace_size is THZ_E_WORKSPACE.
 */
typedef struct thz_ifta_desc {
  long long N;               /* planes */
  int H, W;
  long long target_planes;   /* 1: T [H, W]; N: T [N, H, W] */
  double alpha, beta;        /* thz_ifta_target_project only */
} thz_ifta_desc;
typedef struct thz_ifta_doe_desc {
  long long N;               /* fields, one height map each */
  int H, W;
  int hs, ws;                /* cells */
  long long incident_planes; /* 0: A = 1; 1: A [H, W]; N: A [N, H, W] */
  float wavelength, epsilon;
  int L;                     /* 1 .. THZ_MAX_LUT */
  float lut[THZ_MAX_LUT];
} thz_ifta_doe_desc;
int thz_ifta_target_stats_workspace_size(const thz_ifta_desc* d, size_t* bytes);
int thz_ifta_target_stats(const thz_ifta_desc* d, const void* U, const float* T, const unsigned char* M, double* out,
                          void* workspace, size_t bytes, thz_stream_t stream);
int thz_ifta_target_project(const thz_ifta_desc* d, const void* U, const float* T, const unsigned char* M,
                            const double* scale, void* out, thz_stream_t stream);
int thz_ifta_doe_project(const thz_ifta_doe_desc* d, const void* U, const void* A, const float* q, float* h, int* idx,
                         thz_stream_t stream);

/*
 * Full-wave validator: a 3-D Yee-grid FDTD solver for one dielectric relief on air (thz_fdtd.hip;
 * quantizationawarethzdoe_amd/fdtd.py -- the reference sends its designs to external solvers).  Additive:
 * THZ_ABI_VERSION stays 9, a caller detects the entries by symbol.
 *
 * Cubic cells of side delta, axes (z, y, x) with x fastest; y and x are the height map's H and W and are
 * periodic, z is the optical axis (the wave travels toward +z) and ends in npml cells of CPML on both sides.
 * Nx = W ppc and Ny = H ppc with ppc = pixel / delta a whole number; for H = 1 any Ny >= 1 is legal (the
 * y-invariant problem; Ny = 1 is the 2-D problem exactly).  Units inside: c = 1, lengths in cells, H times
 * eta0, dt = courant cells.  The six fields are float32 [Nz][Ny][Nx]; all cell indexing is 64-bit.
 *
 * The element starts at plane k_elem: n_base cells of base plate, then per pixel floor(clamp(h, 0,
 * thickness) / delta + 1/2) cells of relief (element = 0: no dielectric, the normalisation run).  The host
 * hands over three tables, formed once in fp64 by the caller (fdtd.py; tests/fdtd_ref.py states them):
 *   step_table [n_table][5] fp64   per step: the source's cos and sin times its ramp (float32 values), the
 *                                  DFT's cos and sin, and whether the step is accumulated (non-zero)
 *   cpml [8][npml] float32         (b, c) at the E planes and (b, c) at the H planes of the front slab (plane
 *                                  l), then of the back slab (plane Nz - npml + l)
 *   cacb [10] float32              Ca[n], Cb[n] for n = 0 .. 4 dielectric cells of the four around an edge
 * A current sheet on plane k_src drives Ex (polarization 0) or Ey (1) with 2 courant (Re A cos + Im A sin),
 * A the complex64 [H, W] incident amplitude on the pixel grid (NULL: 1).  The running DFT of Ex, Ey, Ez is
 * summed in fp64, in time order, on n_planes (<= THZ_FDTD_MAX_PLANES) transverse planes plane_k[], on the
 * x-z slice of row `row` and on the y-z slice of column `col` (-1: none).  A device step counter in the
 * workspace selects the table's row; steps past n_table run without source and without accumulation.
 *
 * thz_fdtd_setup      rasterises, clears fields, psi, accumulators and the counter, copies the tables
 * thz_fdtd_run        enqueues 2 n_steps launches (H pass, E pass); no host sync, capturable
 * thz_fdtd_monitors   the accumulators times 2 / n_acc as complex64: planes_out [n_planes][3][Ny][Nx],
 *                     zx_out [3][Nz][Nx], zy_out [3][Nz][Ny]
 * thz_fdtd_fields     out6 [6][Nz][Ny][Nx]: Ex, Ey, Ez, Hx, Hy, Hz as they stand (a hook for tests)
 * thz_fdtd_material   out [Nz][Ny][Nx] uint16: the rasterised word nx | ny << 3 | nz << 6 of edge counts (a hook
 *                     for tests: the rasteriser against the restatement; no product code calls it)
 * Every entry checks before any device call: a null descriptor, pointer or table, a misaligned array, a bad
 * shape, a Courant number outside (0, 1 / sqrt(3)], the source plane, a monitor plane or the element inside
 * a PML slab are THZ_E_ARG; a pixel that is no whole number of cells and a grid beyond the launch extent
 * are THZ_E_UNSUPPORTED; a workspace (256-byte aligned) below thz_fdtd_workspace_size is THZ_E_WORKSPACE.
 */
#define THZ_FDTD_MAX_PLANES 8
typedef struct thz_fdtd_desc {
  int Nz, Ny, Nx;                /* cells */
  int H, W;                      /* pixels of the height map */
  double pixel, delta, courant;
  int npml, k_elem, n_base, element;
  float thickness;
  int k_src, polarization;
  int n_planes;
  int plane_k[THZ_FDTD_MAX_PLANES];
  int row, col;
  long long n_table;
  int n_acc;                     /* accumulated steps: the monitors' scale is 2 / n_acc */
  const double* step_table;      /* host */
  const float* cpml;             /* host */
  const float* cacb;             /* host */
} thz_fdtd_desc;
int thz_fdtd_workspace_size(const thz_fdtd_desc* d, size_t* bytes);
int thz_fdtd_setup(const thz_fdtd_desc* d, const float* height, const void* incident, void* workspace, size_t bytes,
                   thz_stream_t stream);
int thz_fdtd_run(const thz_fdtd_desc* d, void* workspace, size_t bytes, long long n_steps, thz_stream_t stream);
int thz_fdtd_monitors(const thz_fdtd_desc* d, const void* workspace, size_t bytes, void* planes_out, void* zx_out,
                      void* zy_out, thz_stream_t stream);
int thz_fdtd_fields(const thz_fdtd_desc* d, const void* workspace, size_t bytes, float* out6, thz_stream_t stream);
int thz_fdtd_material(const thz_fdtd_desc* d, const void* workspace, size_t bytes, unsigned short* out,
                      thz_stream_t stream);

/*
 * Fabrication-tolerance Monte Carlo: K perturbed realisations of one height map applied to one incident
 * field in one streaming pass (thz_tolerance.hip; quantizationawarethzdoe_amd/tolerance.py).  Additive:
 * THZ_ABI_VERSION stays 9, a caller detects the entries by symbol.  The reference has one term of this
 * model, add_height_map_noise's per-pixel U(-tol, tol) draw (Components/QuantizedDOE.py:82-87).
 *
 * For realisation k (absolute index, first <= k < first + K) and pixel p of the [hs, ws] map with level
 * index l = idx[p], in fp32, in this operation order, contraction off:
 *   u_k[p] = ((1 + g_k) * h[p] + e_{k,l}) + r_k[p]
 *   h_k[p] = min(max(u_k[p], lo), hi)
 *   out[k, c, q] = field[b, c, q] * t_c(h_k[src(q)])      b = 0 for Bf == 1, else k - first
 *   g_k     = sigma_scale * n(THZ_TOL_TAG_SCALE, k)                  a depth-scale error
 *   e_{k,l} = sigma_level[l] * n(THZ_TOL_TAG_LEVEL, 16 k + l)        a per-level depth error; an idx value
 *                                                                    outside 0 .. L-1 takes none
 *   r_k[p]  = ((u - 0.5) * 2) * rough   (THZ_TOL_ROUGH_UNIFORM, the reference's formula)
 *           = rough * n                 (THZ_TOL_ROUGH_NORMAL), drawn at (THZ_TOL_TAG_ROUGH, k hs ws + p)
 * n is thz_noise_draws' THZ_DRAW_NORMAL and u its THZ_DRAW_UNIFORM of (rng, stream ^ tag, index).  A term
 * whose sigma is 0 is not drawn and contributes +0.  t_c is the transmission of thz_doe_modulate_forward
 * (base plate included), src its nearest upsampling, and the complex product is that kernel's, so
 * out[k] == thz_doe_modulate_forward(field, heights_out[k]) bit for bit.  A realisation is a pure function
 * of (seed, step, stream, k, p): it does not depend on first (how K is chunked), on the field size, on the
 * launch geometry or on whether the 16-byte path ran (all pointers 16-byte aligned and H W % 4 == 0) or the
 * element-width one.
 *
 * field [Bf, C, H, W] complex64 with Bf = 1 or K; height [hs, ws] float32; idx [hs, ws] int32 or NULL (legal
 * only when every sigma_level is 0); out [K, C, H, W] complex64; heights_out [K, hs, ws] float32 or NULL.
 *
 * thz_tolerance_modulate_backward, for the cotangent G = grad_out [K, C, H, W], every draw regenerated:
 *   grad_height[p] = sum_k (1 + g_k) [lo < u_k[p] < hi] sum_c sum_{q: src(q) = p}
 *                    Re(conj(G[k,c,q]) field[b,c,q] t_c(h_k[p]) gamma_c)              float32 [hs, ws], or NULL
 *   grad_field     = G conj(t), summed over k when Bf == 1                          complex64 [Bf, C, H, W], or NULL
 * One thread owns a map pixel and the field pixels that read it, and sums in fp64 in the fixed order
 * (c, q row-major, k): no atomics, the same bits from every call and every grid.  It needs no workspace
 * today (workspace may be NULL and bytes 0; the parameters are reserved).
 *
 * Checked on the host before any device call: null pointers, a shape below 1, Bf other than 1 or K, L outside
 * 0 .. THZ_MAX_LUT, a negative or NaN sigma or roughness, an unknown roughness kind, lo > hi or a NaN bound,
 * first < 0, (first + K) hs ws > 2^32 or (first + K) 16 > 2^32 (the generator's index is 32-bit), idx == NULL
 * with a non-zero sigma_level, and misaligned arrays are THZ_E_ARG; C > THZ_MAX_WAVELENGTHS is
 * THZ_E_UNSUPPORTED.
 */
#define THZ_TOL_TAG_SCALE 0x5343414Cu /* "SCAL" */
#define THZ_TOL_TAG_LEVEL 0x4C45564Cu /* "LEVL" */
#define THZ_TOL_TAG_ROUGH 0x524F5547u /* "ROUG" */
#define THZ_TOL_ROUGH_NONE 0
#define THZ_TOL_ROUGH_UNIFORM 1
#define THZ_TOL_ROUGH_NORMAL 2
typedef struct thz_tolerance_desc {
  int K;                     /* realisations of this call */
  long long first;           /* absolute index of the first */
  int Bf;                    /* batch items of field: 1 or K */
  int C, H, W, hs, ws;
  int L;                     /* entries of sigma_level, 0 .. THZ_MAX_LUT */
  float sigma_level[THZ_MAX_LUT];
  float sigma_scale;
  int rough_kind;            /* THZ_TOL_ROUGH_* */
  float rough;
  float lo, hi;              /* clamp; -inf / +inf switch a side off */
  float epsilon, tand;
  const float* wavelengths;  /* host [C] */
  const unsigned* rng;       /* device [2] = {seed, step} */
  unsigned stream;
} thz_tolerance_desc;
int thz_tolerance_modulate_forward(const thz_tolerance_desc* d, const void* field, const float* height, const int* idx,
                                   void* out, float* heights_out, thz_stream_t stream);
int thz_tolerance_modulate_backward(const thz_tolerance_desc* d, const void* grad_out, const void* field,
                                    const float* height, const int* idx, void* grad_field, float* grad_height,
                                    void* workspace, size_t bytes, thz_stream_t stream);

/*
 * Batched 1-D FFT along the contiguous axis (the building block of ft2/ift2,
 * utils/Helper_Functions.py:150, without shifts): in/out [rows, n], unnormalised,
 * inverse != 0 for the backward transform.  n <= 16384, any factorisation.
 */
int thz_fft_rows(const void* in, void* out, int rows, int n, int inverse, thz_stream_t stream);

/*
 * Double precision (complex128).  The reference computes in the field's precision: a complex128
 * field or float64 wavelength tensor runs ASM / CZT / RSC in fp64 and returns complex128
 * (DataType/ElectricField.py:85-90; test_czt.py:12 runs RSC + CZT that way).  These entries are
 * the fp32 ones with double scalars and complex128 buffers (interleaved double (re, im), identical
 * to torch.complex128); same shapes, windows and error codes.  Transform lengths (padded sizes,
 * Bluestein np2) up to 8192.  The fp64 ASM adjoint takes one z-plane (Z == 1).
 */
typedef struct thz_asm_desc64 {
  int B, C, H, W;
  int pad_h, pad_w;
  int unpad;
  int bandlimit;             /* THZ_BANDLIMIT_* */
  int Z;                     /* 1 .. THZ_MAX_Z; 1 for the adjoint */
  int adjoint;
  double dx, dy;
  const double* wavelengths; /* host [C] */
  const double* z;           /* host [Z] */
} thz_asm_desc64;
int thz_asm64_workspace_size(const thz_asm_desc64* d, size_t* bytes);
int thz_asm64_forward(const thz_asm_desc64* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
                      thz_stream_t stream);

typedef struct thz_czt_desc64 {
  int B, C, H, W;
  int outH, outW;
  double dx, dy;
  double odx, ody;
  double z;
  const double* wavelengths; /* host [C] */
  int adjoint;
} thz_czt_desc64;
int thz_czt64_workspace_size(const thz_czt_desc64* d, size_t* bytes);
int thz_czt64_forward(const thz_czt_desc64* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
                      thz_stream_t stream);

typedef struct thz_rsc_desc64 {
  int B, C, H, W;
  int vectorial;
  double dx, dy;
  double z;
  const double* wavelengths; /* host [C] */
  int adjoint;
} thz_rsc_desc64;
int thz_rsc64_workspace_size(const thz_rsc_desc64* d, size_t* bytes);
int thz_rsc64_forward(const thz_rsc_desc64* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
                      thz_stream_t stream);

/* Batched 1-D FFT of complex128 rows (as thz_fft_rows), n <= 8192. */
int thz_fft64_rows(const void* in, void* out, int rows, int n, int inverse, thz_stream_t stream);

/* thz_stokes_forward / thz_polarization_ellipse (Addons/Polarization.py:45-92) on complex128 planes
 * with double outputs [4][n]; same validation, eps and clamp. */
int thz_stokes64_forward(const void* ex, const void* ey, long long n, double* out, thz_stream_t stream);
int thz_polarization_ellipse64(const void* ex, const void* ey, long long n, double* out, thz_stream_t stream);

/*
 * Per-step state of the graph-replayed trainers (not part of the reference: qat.py StepState, the
 * schedule values tau / s / beta, the device generator's seed and step, the multi-plane systems'
 * plane distances, as int32 bit patterns).  ring: [depth][width] int32 in pinned host memory
 * (hipHostMalloc'd, device-mapped), one slot filled by the host per replay; counter: device int32 [1],
 * the fetches so far.  Copies slot (counter mod depth) into state (device [width] int32) and
 * increments counter -- a step's graph captures it as its first node, so every replay reads the
 * slot its host call filled without a host->device copy command between replays.  The caller
 * rewrites a slot only after the replay that read it has run.  1 <= width <= 5 + THZ_MAX_Z.
 */
int thz_step_fetch(const int* ring, int depth, int width, int* state, int* counter, thz_stream_t stream);

/*
 * One Adam / AdamW step over up to THZ_MAX_ADAM_PARAMS fp32 parameters in one launch (the trainers'
 * optimiser, quantizationawarethzdoe_amd/optim.py; the reference's notebooks step torch.optim.Adam /
 * AdamW, e.g. plot_data/example_1/experiment_four_focal_spots.ipynb cells 22, 33, 52).  Per element,
 * torch's single-tensor update with t = *step + 1 (each parameter's own device step count,
 * incremented by the launch); the scalars (1 - b1, 1 - b2, 1 - lr wd, the bias corrections) formed
 * in fp64 and rounded to fp32, as torch forms them in Python:
 *   decoupled (AdamW): p *= 1 - lr wd;   else g += wd p
 *   m = lerp(m, g, 1 - b1);   v = v b2 + (1 - b2) g g
 *   p += -(lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * done: device u32 [1], zero before the first launch (the launch leaves it zero): the last
 * workgroup to finish advances the step counts, after every workgroup has read them.
 */
#define THZ_MAX_ADAM_PARAMS 16
typedef struct thz_adam_param {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* step;      /* device [1] */
  long long n;      /* elements */
} thz_adam_param;
typedef struct thz_adam_desc {
  double lr, beta1, beta2, eps, weight_decay;
  int decoupled;    /* 1: AdamW */
  int nparams;      /* 1 .. THZ_MAX_ADAM_PARAMS */
  unsigned* done;   /* device [1] */
} thz_adam_desc;
int thz_adam_step(const thz_adam_desc* d, const thz_adam_param* params, thz_stream_t stream);

/*
 * Per-kernel HIP-event timing used by bench.py (not part of the reference): when
 * enabled every kernel launch is bracketed by two events on its own stream;
 * thz_timing_read() synchronises on the pending events and returns the summed
 * duration and launch count for one kernel name ("asm_rows_fwd", "asm_cols", "asm_rows_inv"; the
 * z-x slice: "asm_rows_fwd", "asm_cols_slice", "asm_rows_slice"; its adjoint: "asm_rows_fwd",
 * "asm_cols_slice_adj", "asm_rows_inv"; the CZT z-x slice: "czt_slice_tables", "czt_slice_collapse",
 * "czt_slice_line"; its adjoint: "czt_slice_tables", "czt_slice_line_adj", "czt_slice_expand"; the
 * RSC z-x slice: "rsc_slice_rows", "rsc_slice_acc", "rsc_slice_line"; its adjoint: "rsc_slice_line_adj",
 * "rsc_slice_acc_adj", "rsc_slice_rows_adj"; the polarization entries: "stokes_fwd", "stokes_bwd",
 * "polarization_ellipse", "stokes64_fwd", "polarization_ellipse64"; the noise entries: "noise_apply",
 * "noise_draws", "signal_scale_part", "signal_scale_finish", "snr_noise_bwd_part", "snr_noise_bwd_finish",
 * "snr_noise_bwd"; the loss entries: "dice_bce_sums", "dice_bce_finish", "dice_bce_bwd", "ssim_fwd",
 * "ssim_finish", "ssim_bwd"; the height-map entries: "lut_quantize_fwd", "lut_quantize_bwd", "center_difference",
 * "tv_fwd", "tv_finish", "tv_bwd", "center_difference_bwd"; the metrics entries: "region_stats_fwd",
 * "region_stats_finish", "region_stats_bwd", "line_widths"; the tolerance entries: "tolerance_fwd",
 * "tolerance_heights", "tolerance_bwd"; ...).
 */
int thz_timing_enable(int on);
int thz_timing_reset(void);
int thz_timing_read(const char* kernel, double* total_ms, long* launches);

#ifdef __cplusplus
}
#endif
#endif /* THZDOE_H_ */
