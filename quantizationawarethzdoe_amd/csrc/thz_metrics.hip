// Focal-spot figures of merit (utils/metrics.py; the reference's utils/metrics.py is an empty
// placeholder, its notebooks grade a design by eye): region statistics of intensity planes and the
// widths of lines, as fused kernels.
//
//   thz_region_stats_forward   one pass over N planes of H x W (complex64 / complex128 fields, I = re^2 + im^2
//                              formed in fp64, or float32 / float64 intensities): for up to 16 circular /
//                              rectangular regions and the whole plane, the sums of I, I i, I j, I i^2, I j^2,
//                              the peak, its lowest flat index and the pixel count.  A workgroup owns a
//                              256-column x 32-row tile (a wave eight rows, a lane four consecutive columns
//                              of each), holds its 32 intensities in registers and visits only the regions
//                              whose bounding box meets the tile, so an element is read once however many
//                              regions there are.  The workgroup's result per region goes to the workspace
//                              (block_reduce_fixed on the whole struct); region_stats_finish_kernel
//                              merges a plane's tiles in index order.  No atomics: the same input gives the
//                              same bits.
//   thz_region_stats_backward  one pass on the same tiles: grad_I = sum over the regions that hold the
//                              pixel of G0 + G1 i + G2 j + G3 i^2 + G4 j^2, written as grad_I (intensities)
//                              or 2 grad_I E (fields) in the input's type.
//   thz_line_widths            peak, lowest argmax and the nearest crossings of level x peak on either
//                              side of it, for L lines of W samples: a wave per line up to
//                              LW_WAVE_MAX samples, a workgroup per line beyond.
// fp64 throughout, contraction off: I, the products I i .. I j^2 and the region tests are the roundings
// of the separate multiplies and adds an fp64 restatement makes.
#include <cstdint>
#include <initializer_list>

#include "thz_common.hpp"
#include "thz_dev.hpp"
#include "thz_stream.hpp"
#include "thz_launch.hpp"

namespace thz {

#pragma clang fp contract(off)

constexpr int RS_THREADS = 256;
constexpr int RS_PX = 4;                      // consecutive columns per lane
constexpr int RS_COLS = 64 * RS_PX;           // a workgroup's tile: 256 columns ...
constexpr int RS_WAVE_ROWS = 8;               // ... by 8 rows per wave,
constexpr int RS_WAVES = RS_THREADS / 64;     //
constexpr int RS_ROWS = RS_WAVE_ROWS * RS_WAVES;  // 32 rows in all
constexpr int RS_MAX_EDGE = 1 << 30;          // rows / columns: a tile's end stays an int
constexpr int RS_STATS = 8;
// three waves per SIMD: 32 fp64 intensities and a region's accumulators fit 168 VGPRs without scratch
#define RS_OCC __attribute__((amdgpu_waves_per_eu(3, 3)))

struct RsShape {
  long long N;
  int H, W;
  int tx, ty;  // tiles across and down a plane
  int K;
  bool wide;   // rows start 16-byte aligned: every base pointer and the row pitch in bytes
};

// the region table: by value (a host table) or read from device memory
struct RsTable {
  const thz_region* dev;  // non-null: the table lives on the device
  thz_region host[THZ_MAX_REGIONS];
};

// a region with its bounding box (inclusive, clipped to the plane; r1 < r0 or c1 < c0: no pixel).
// kind < 0: the whole plane.
struct RsBox {
  int kind;
  int r0, r1, c0, c1;
  double cr, cc, a, b;
};

// floor / ceil of a bound clipped to [lo, hi]; NaN gives `nan`
__device__ __forceinline__ int rs_clip(double v, int lo, int hi, int nan) {
  if (v != v) return nan;
  if (v <= (double)lo) return lo;
  if (v >= (double)hi) return hi;
  return (int)v;  // lo < v < hi: in the int range
}

__device__ __forceinline__ RsBox rs_box(const RsTable& tab, const RsShape& s, int k) {
  RsBox x;
  if (k >= s.K) {
    x.kind = -1;
    x.r0 = 0; x.r1 = s.H - 1; x.c0 = 0; x.c1 = s.W - 1;
    x.cr = x.cc = x.a = x.b = 0.0;
    return x;
  }
  const thz_region r = tab.dev ? tab.dev[k] : tab.host[k];
  x.kind = r.kind == THZ_REGION_CIRC ? THZ_REGION_CIRC : THZ_REGION_RECT;
  x.cr = (double)r.cr; x.cc = (double)r.cc; x.a = (double)r.a; x.b = (double)r.b;
  // circ: |d| <= |a| on each axis; rect: a negative half-size holds no pixel (lo > hi below)
  const double hr = x.kind == THZ_REGION_CIRC ? fabs(x.a) : x.a;
  const double hc = x.kind == THZ_REGION_CIRC ? fabs(x.a) : x.b;
  // one row / column of slack either way: the box only prunes, the fp64 test decides
  x.r0 = rs_clip(floor(x.cr - hr), 0, s.H, s.H);
  x.r1 = rs_clip(ceil(x.cr + hr), -1, s.H - 1, -1);
  x.c0 = rs_clip(floor(x.cc - hc), 0, s.W, s.W);
  x.c1 = rs_clip(ceil(x.cc + hc), -1, s.W - 1, -1);
  return x;
}

__device__ __forceinline__ bool rs_hits(const RsBox& x, int r0, int r1, int c0, int c1) {  // inclusive ranges
  return x.r0 <= r1 && x.r1 >= r0 && x.c0 <= c1 && x.c1 >= c0;
}

// the boxes of regions 0 .. K in LDS; every thread calls it
__device__ __forceinline__ void rs_boxes(const RsTable& tab, const RsShape& s, RsBox* s_box) {
  if ((int)threadIdx.x <= s.K) s_box[threadIdx.x] = rs_box(tab, s, threadIdx.x);
  __syncthreads();
}

// a workgroup's tile and its lane's four columns of the wave's eight rows
struct RsTile {
  long long plane;  // element offset of the plane
  long long slot;   // index of the tile's partials: n ty tx + tile
  int R0, C0;       // the workgroup's first row and column
  int r0, c0;       // the wave's first row, the lane's first column
  __device__ __forceinline__ RsTile(const RsShape& s) {
    slot = blockIdx.x;
    const long long per = (long long)s.tx * s.ty, n = slot / per, rem = slot - n * per;
    plane = n * s.H * s.W;
    R0 = (int)(rem / s.tx) * RS_ROWS;  // < H and C0 < W: ints by rs_shape's bound on H, W
    C0 = (int)(rem % s.tx) * RS_COLS;
    r0 = R0 + (threadIdx.x >> 6) * RS_WAVE_ROWS;
    c0 = C0 + (threadIdx.x & 63) * RS_PX;
  }
};

template <class T> struct RsElem;
template <> struct RsElem<float> {
  static constexpr bool field = false;
  static __device__ __forceinline__ double inten(float v) { return (double)v; }
};
template <> struct RsElem<double> {
  static constexpr bool field = false;
  static __device__ __forceinline__ double inten(double v) { return v; }
};
template <> struct RsElem<float2> {
  static constexpr bool field = true;
  static __device__ __forceinline__ double inten(float2 v) {
    const double x = (double)v.x, y = (double)v.y;
    return x * x + y * y;
  }
};
template <> struct RsElem<double2> {
  static constexpr bool field = true;
  static __device__ __forceinline__ double inten(double2 v) { return v.x * v.x + v.y * v.y; }
};
__device__ __forceinline__ float rs_scale(float v, double g) { return (float)g; }
__device__ __forceinline__ double rs_scale(double v, double g) { return g; }
__device__ __forceinline__ float2 rs_scale(float2 v, double g) {
  return make_float2((float)(2.0 * g * (double)v.x), (float)(2.0 * g * (double)v.y));
}
__device__ __forceinline__ double2 rs_scale(double2 v, double g) { return make_double2(2.0 * g * v.x, 2.0 * g * v.y); }

// the lane's four elements of row i (i < H), zero past the row's end
template <class T>
__device__ __forceinline__ void rs_load(const T* __restrict__ p, const RsShape& s, const RsTile& t, int i, T v[RS_PX]) {
  ld4(p + t.plane + (long long)i * s.W, t.c0, s.W, s.wide, v);
}
template <class T>
__device__ __forceinline__ void rs_store(T* __restrict__ p, const RsShape& s, const RsTile& t, int i, const T v[RS_PX]) {
  st4(p + t.plane + (long long)i * s.W, t.c0, s.W, s.wide, v);
}

// the statistics of one region over some pixels
struct RsAcc {
  double s0, sr, sc, srr, scc, peak, cnt;
  long long arg;
  __device__ __forceinline__ void clear() {
    s0 = sr = sc = srr = scc = cnt = 0.0;
    peak = -__builtin_inf();
    arg = INT64_MAX;
  }
  // pixels are added in ascending flat index within a lane: the strict test keeps the lowest.
  // loc: the number of the lane's pixel that holds the peak so far
  __device__ __forceinline__ void add(double I, double di, double dj, double dii, double djj, int& loc, int id) {
    s0 += I;
    sr += I * di;
    sc += I * dj;
    srr += I * dii;
    scc += I * djj;
    cnt += 1.0;
    if (I > peak) {
      peak = I;
      loc = id;
    }
  }
  __device__ __forceinline__ void merge(const RsAcc& o) {
    s0 += o.s0; sr += o.sr; sc += o.sc; srr += o.srr; scc += o.scc; cnt += o.cnt;
    if (o.peak > peak || (o.peak == peak && o.arg < arg)) {
      peak = o.peak;
      arg = o.arg;
    }
  }
  __device__ __forceinline__ RsAcc shfl_xor(int o) const {  // for block_reduce_fixed
    RsAcc b;
    b.s0 = __shfl_xor(s0, o); b.sr = __shfl_xor(sr, o); b.sc = __shfl_xor(sc, o);
    b.srr = __shfl_xor(srr, o); b.scc = __shfl_xor(scc, o); b.peak = __shfl_xor(peak, o);
    b.cnt = __shfl_xor(cnt, o); b.arg = __shfl_xor(arg, o);
    return b;
  }
  __device__ __forceinline__ void store(double* o) const {
    const bool any = cnt > 0.0;
    o[0] = s0; o[1] = sr; o[2] = sc; o[3] = srr; o[4] = scc;
    o[5] = any && arg != INT64_MAX ? peak : 0.0;  // NaN never wins a comparison: a region of NaN alone has no peak
    o[6] = any && arg != INT64_MAX ? (double)arg : -1.0;
    o[7] = cnt;
  }
  static __device__ __forceinline__ RsAcc of(const double* o) {
    RsAcc a;
    a.s0 = o[0]; a.sr = o[1]; a.sc = o[2]; a.srr = o[3]; a.scc = o[4];
    a.cnt = o[7];
    const bool any = o[6] >= 0.0;
    a.peak = any ? o[5] : -__builtin_inf();
    a.arg = any ? (long long)o[6] : INT64_MAX;
    return a;
  }
};

// is pixel (i, j) inside?  dii = (i - cr)^2 for a circle, |i - cr| for a rectangle; djj alike
__device__ __forceinline__ bool rs_member(const RsBox& x, double dii, double djj, double aa) {
  if (x.kind < 0) return true;
  if (x.kind == THZ_REGION_CIRC) return dii + djj <= aa;
  return dii <= x.a && djj <= x.b;
}
__device__ __forceinline__ double rs_axis(const RsBox& x, int i, double c) {
  const double d = (double)i - c;
  return x.kind == THZ_REGION_CIRC ? d * d : fabs(d);
}

// partial[(slot (K + 1) + k) 8 ..]: region k over the workgroup's tile, written only where the
// region's box meets the tile (the finish kernel makes the same test)
template <class T>
__global__ void __launch_bounds__(RS_THREADS) RS_OCC region_stats_fwd_kernel(RsShape s, RsTable tab, const T* __restrict__ x,
                                                                      double* __restrict__ partial) {
  __shared__ RsBox s_box[THZ_MAX_REGIONS + 1];
  rs_boxes(tab, s, s_box);
  const RsTile t(s);
  double I[RS_WAVE_ROWS][RS_PX];
#pragma unroll
  for (int r = 0; r < RS_WAVE_ROWS; ++r) {
    T v[RS_PX];
    if (t.r0 + r < s.H) {  // wave-uniform
      rs_load(x, s, t, t.r0 + r, v);
#pragma unroll
      for (int k = 0; k < RS_PX; ++k) I[r][k] = RsElem<T>::inten(v[k]);
    } else {
#pragma unroll
      for (int k = 0; k < RS_PX; ++k) I[r][k] = 0.0;
    }
  }
  const int wr1 = t.r0 + RS_WAVE_ROWS - 1, wc0 = t.C0, wc1 = t.C0 + RS_COLS - 1;
  for (int k = 0; k <= s.K; ++k) {
    const RsBox b = s_box[k];
    if (!rs_hits(b, t.R0, t.R0 + RS_ROWS - 1, wc0, wc1)) continue;  // workgroup-uniform
    RsAcc acc;
    acc.clear();
    if (rs_hits(b, t.r0, wr1, wc0, wc1)) {  // wave-uniform
      // The coordinates are formed anew for every region (a few conversions and multiplies): left to itself
      // the compiler hoists i, i^2, j, j^2 and the flat index of all 32 pixels out of the region loop and
      // spills.  The empty statement makes r0 and c0 opaque; the peak is tracked by the pixel's number in
      // the lane (a compile-time constant) and turned into the flat index once.
      int r0 = t.r0, c0 = t.c0;
      asm volatile("" : "+v"(r0), "+v"(c0));
      const double aa = b.a * b.a;
      double djj[RS_PX], dj[RS_PX];
#pragma unroll
      for (int q = 0; q < RS_PX; ++q) {
        djj[q] = rs_axis(b, c0 + q, b.cc);
        dj[q] = (double)(c0 + q);
      }
      int loc = -1;
#pragma unroll
      for (int r = 0; r < RS_WAVE_ROWS; ++r) {
        const int i = r0 + r;
        const double dii = rs_axis(b, i, b.cr), di = (double)i, di2 = di * di;
#pragma unroll
        for (int q = 0; q < RS_PX; ++q)
          if (i < s.H && c0 + q < s.W && rs_member(b, dii, djj[q], aa))
            acc.add(I[r][q], di, dj[q], di2, dj[q] * dj[q], loc, r * RS_PX + q);
      }
      if (loc >= 0) acc.arg = (long long)(r0 + loc / RS_PX) * s.W + (c0 + loc % RS_PX);
    }
    acc = block_reduce_fixed(acc);
    if (threadIdx.x == 0) acc.store(partial + ((size_t)t.slot * (s.K + 1) + k) * RS_STATS);
  }
}

// out[(n (K + 1) + k) 8 ..]: one workgroup per plane and region merges the plane's tiles, each thread
// its tiles in ascending order (gather_reduce)
__global__ void __launch_bounds__(RS_THREADS) region_stats_finish_kernel(RsShape s, RsTable tab,
                                                                         const double* __restrict__ partial,
                                                                         double* __restrict__ out) {
  const long long n = blockIdx.x / (s.K + 1);
  const int k = (int)(blockIdx.x - n * (s.K + 1));
  const RsBox b = rs_box(tab, s, k);
  const long long per = (long long)s.tx * s.ty;
  RsAcc acc;
  acc.clear();
  acc = gather_reduce(acc, per, [&](long long tile, RsAcc& a) {
    const int R0 = (int)(tile / s.tx) * RS_ROWS, C0 = (int)(tile % s.tx) * RS_COLS;
    if (!rs_hits(b, R0, R0 + RS_ROWS - 1, C0, C0 + RS_COLS - 1)) return;
    a.merge(RsAcc::of(partial + ((size_t)(n * per + tile) * (s.K + 1) + k) * RS_STATS));
  });
  if (threadIdx.x == 0) acc.store(out + (size_t)blockIdx.x * RS_STATS);
}

// G [N, K + 1, 5]: the cotangents of S0, Sr, Sc, Srr, Scc
template <class T>
__global__ void __launch_bounds__(RS_THREADS) RS_OCC region_stats_bwd_kernel(RsShape s, RsTable tab, const T* __restrict__ x,
                                                                      const double* __restrict__ G,
                                                                      T* __restrict__ grad) {
  __shared__ RsBox s_box[THZ_MAX_REGIONS + 1];
  rs_boxes(tab, s, s_box);
  const RsTile t(s);
  if (t.r0 >= s.H) return;  // wave-uniform; no barrier below
  const long long n = t.slot / ((long long)s.tx * s.ty);
  double g[RS_WAVE_ROWS][RS_PX];
#pragma unroll
  for (int r = 0; r < RS_WAVE_ROWS; ++r)
#pragma unroll
    for (int q = 0; q < RS_PX; ++q) g[r][q] = 0.0;
  const int wr1 = t.r0 + RS_WAVE_ROWS - 1, wc0 = t.C0, wc1 = t.C0 + RS_COLS - 1;
  for (int k = 0; k <= s.K; ++k) {
    const RsBox b = s_box[k];
    if (!rs_hits(b, t.r0, wr1, wc0, wc1)) continue;  // wave-uniform
    const double* gk = G + ((size_t)n * (s.K + 1) + k) * 5;
    const double g0 = gk[0], g1 = gk[1], g2 = gk[2], g3 = gk[3], g4 = gk[4];
    const double aa = b.a * b.a;
    double djj[RS_PX], cj[RS_PX];
#pragma unroll
    for (int q = 0; q < RS_PX; ++q) {
      const double dj = (double)(t.c0 + q);
      djj[q] = rs_axis(b, t.c0 + q, b.cc);
      cj[q] = g2 * dj + g4 * (dj * dj);
    }
#pragma unroll
    for (int r = 0; r < RS_WAVE_ROWS; ++r) {
      const int i = t.r0 + r;
      const double dii = rs_axis(b, i, b.cr), di = (double)i, ci = g0 + g1 * di + g3 * (di * di);
#pragma unroll
      for (int q = 0; q < RS_PX; ++q)
        if (rs_member(b, dii, djj[q], aa)) g[r][q] += ci + cj[q];
    }
  }
#pragma unroll
  for (int r = 0; r < RS_WAVE_ROWS; ++r) {
    const int i = t.r0 + r;
    if (i >= s.H) break;
    T v[RS_PX], o[RS_PX];
    if constexpr (RsElem<T>::field) {
      rs_load(x, s, t, i, v);
    } else {
#pragma unroll
      for (int q = 0; q < RS_PX; ++q) v[q] = T{};
    }
#pragma unroll
    for (int q = 0; q < RS_PX; ++q) o[q] = rs_scale(v[q], g[r][q]);
    rs_store(grad, s, t, i, o);
  }
}

// ---- line widths -----------------------------------------------------------------------------
constexpr int LW_THREADS = 256;
constexpr int LW_WAVES = LW_THREADS / 64;
constexpr int LW_WAVE_MAX = 1024;  // samples up to which a wave takes a line

// out[line 5 ..] = peak, argmax, xl, xr, xr - xl.  PER_WAVE: line = 4 workgroup + wave, no barrier;
// else line = workgroup
template <class T, bool PER_WAVE>
__global__ void __launch_bounds__(LW_THREADS) line_widths_kernel(const T* __restrict__ v, long long L, int W, double f,
                                                                 double* __restrict__ out) {
  __shared__ double s_pk[LW_WAVES];
  __shared__ int s_a[LW_WAVES], s_l[LW_WAVES], s_r[LW_WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long long line = PER_WAVE ? (long long)blockIdx.x * LW_WAVES + wid : (long long)blockIdx.x;
  if (PER_WAVE && line >= L) return;  // wave-uniform
  const int tid = PER_WAVE ? lane : (int)threadIdx.x, step = PER_WAVE ? 64 : LW_THREADS;
  const T* p = v + line * W;
  double pk = -__builtin_inf();
  int arg = INT32_MAX;
  for (int j = tid; j < W; j += step) {  // ascending j: the strict test keeps the lowest
    const double val = (double)p[j];
    if (val > pk) {
      pk = val;
      arg = j;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double opk = __shfl_xor(pk, o);
    const int oarg = __shfl_xor(arg, o);
    if (opk > pk || (opk == pk && oarg < arg)) {
      pk = opk;
      arg = oarg;
    }
  }
  if (!PER_WAVE) {
    if (lane == 0) {
      s_pk[wid] = pk;
      s_a[wid] = arg;
    }
    __syncthreads();
    pk = s_pk[0];
    arg = s_a[0];
    for (int w = 1; w < LW_WAVES; ++w)
      if (s_pk[w] > pk || (s_pk[w] == pk && s_a[w] < arg)) {
        pk = s_pk[w];
        arg = s_a[w];
      }
  }
  if (arg == INT32_MAX) {  // no sample compares above -inf (NaN throughout)
    if (tid == 0) {
      double* o = out + line * 5;
      const double q = __builtin_nan("");
      o[0] = q; o[1] = 0.0; o[2] = q; o[3] = q; o[4] = q;
    }
    return;  // uniform over the line's threads
  }
  const double thr = f * pk;
  int jl = -1, jr = W;  // the largest index below the peak's, the smallest above it, with v < thr
  for (int j = tid; j < W; j += step) {
    if (j == arg) continue;
    if ((double)p[j] < thr) {
      if (j < arg) jl = j;                   // ascending j: the last is the largest
      else if (jr == W) jr = j;              // the first is the smallest
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int ol = __shfl_xor(jl, o), orr = __shfl_xor(jr, o);
    jl = ol > jl ? ol : jl;
    jr = orr < jr ? orr : jr;
  }
  if (!PER_WAVE) {
    if (lane == 0) {
      s_l[wid] = jl;
      s_r[wid] = jr;
    }
    __syncthreads();
    for (int w = 0; w < LW_WAVES; ++w) {
      jl = s_l[w] > jl ? s_l[w] : jl;
      jr = s_r[w] < jr ? s_r[w] : jr;
    }
  }
  if (tid == 0) {
    double xl = __builtin_nan(""), xr = __builtin_nan("");
    if (jl >= 0) {
      const double v0 = (double)p[jl], v1 = (double)p[jl + 1];
      xl = (double)jl + (thr - v0) / (v1 - v0);
    }
    if (jr < W) {
      const double v0 = (double)p[jr], v1 = (double)p[jr - 1];
      xr = (double)jr - (thr - v0) / (v1 - v0);
    }
    double* o = out + line * 5;
    o[0] = pk; o[1] = (double)arg; o[2] = xl; o[3] = xr; o[4] = xr - xl;
  }
}

#pragma clang fp contract(on)

// ---- host side -------------------------------------------------------------------------------
static size_t elem_bytes(int dtype) {
  switch (dtype) {
    case THZ_METRICS_C64: return 8;
    case THZ_METRICS_C128: return 16;
    case THZ_METRICS_F32: return 4;
    case THZ_METRICS_F64: return 8;
  }
  return 0;
}
// the alignment of an element's components
static size_t comp_bytes(int dtype) { return dtype == THZ_METRICS_C64 || dtype == THZ_METRICS_F32 ? 4 : 8; }

static int rs_shape(const char* who, const thz_region_stats_desc* d, RsShape* s, RsTable* tab) {
  if (!d) return fail(THZ_E_ARG, "%s: null descriptor", who);
  if (d->N < 0 || d->H < 0 || d->W < 0)
    return fail(THZ_E_ARG, "%s: bad shape N = %lld, H = %d, W = %d", who, d->N, d->H, d->W);
  if (d->K < 0 || d->K > THZ_MAX_REGIONS) return fail(THZ_E_ARG, "%s: %d regions (0 .. %d)", who, d->K, THZ_MAX_REGIONS);
  if (!elem_bytes(d->dtype)) return fail(THZ_E_ARG, "%s: dtype %d", who, d->dtype);
  if (d->K > 0 && !d->regions) return fail(THZ_E_ARG, "%s: null region table", who);
  if (d->H > RS_MAX_EDGE || d->W > RS_MAX_EDGE)
    return fail(THZ_E_UNSUPPORTED, "%s: H = %d, W = %d beyond 2^30 rows / columns", who, d->H, d->W);
  s->N = d->N; s->H = d->H; s->W = d->W; s->K = d->K;
  s->tx = (d->W + RS_COLS - 1) / RS_COLS;
  s->ty = (d->H + RS_ROWS - 1) / RS_ROWS;
  s->wide = false;
  const long long per = (long long)s->tx * s->ty, most = per > d->K + 1 ? per : d->K + 1;  // the two grids
  if (d->N > ((1LL << 31) - 1) / most)
    return fail(THZ_E_UNSUPPORTED, "%s: N = %lld planes of %d x %d beyond the grid's extent", who, d->N, d->H, d->W);
  *tab = RsTable{};
  if (d->regions_on_device) {
    if (d->K > 0) {
      if (misaligned(d->regions, 4)) return fail(THZ_E_ARG, "%s: region table not 4-byte aligned", who);
      tab->dev = d->regions;
    }
  } else {
    for (int k = 0; k < d->K; ++k) {
      const thz_region& r = d->regions[k];
      if (r.kind != THZ_REGION_CIRC && r.kind != THZ_REGION_RECT)
        return fail(THZ_E_ARG, "%s: region %d has kind %d", who, k, r.kind);
      tab->host[k] = r;
    }
  }
  return THZ_OK;
}
static long long rs_tiles(const RsShape& s) { return s.N * s.tx * s.ty; }
static size_t rs_workspace(const RsShape& s) {
  return align256(sizeof(double) * RS_STATS * (size_t)(s.K + 1) * (size_t)rs_tiles(s));
}
// every row starts 16-byte aligned when the base pointers do
static bool rs_pitch16(const RsShape& s, int dtype) { return ((size_t)s.W * elem_bytes(dtype)) % 16 == 0; }

// f(T{}) with the element type of dtype
template <class F>
static void on_dtype(int dtype, F&& f) {
  switch (dtype) {
    case THZ_METRICS_C64: f(float2{}); break;
    case THZ_METRICS_C128: f(double2{}); break;
    case THZ_METRICS_F32: f(float{}); break;
    default: f(double{}); break;
  }
}

}  // namespace thz

using namespace thz;

extern "C" int thz_region_stats_workspace_size(const thz_region_stats_desc* d, size_t* bytes) {
  const char* who = "thz_region_stats_workspace_size";
  if (!bytes) return fail(THZ_E_ARG, "%s: null pointer", who);
  RsShape sh;
  RsTable tab;
  if (int e = rs_shape(who, d, &sh, &tab)) return e;
  *bytes = rs_workspace(sh);
  return THZ_OK;
}

extern "C" int thz_region_stats_forward(const thz_region_stats_desc* d, const void* x, double* out, void* workspace,
                                        size_t bytes, thz_stream_t stream) {
  const char* who = "thz_region_stats_forward";
  RsShape sh;
  RsTable tab;
  if (int e = rs_shape(who, d, &sh, &tab)) return e;
  if (d->N == 0) return THZ_OK;
  if (!out || misaligned(out, sizeof(double))) return fail(THZ_E_ARG, "%s: out null or misaligned", who);
  if (workspace && misaligned(workspace, sizeof(double))) return fail(THZ_E_ARG, "%s: workspace misaligned", who);
  hipStream_t s = (hipStream_t)stream;
  const dim3 b(RS_THREADS);
  if (rs_tiles(sh) > 0) {  // H or W == 0: no pixel, the finish kernel alone writes the empty statistics
    if (!x || misaligned(x, comp_bytes(d->dtype))) return fail(THZ_E_ARG, "%s: x null or misaligned", who);
    if (int e = check_workspace(workspace, bytes, rs_workspace(sh))) return e;
    sh.wide = rs_pitch16(sh, d->dtype) && all_aligned16({x});
    KernelTimer kt("region_stats_fwd", s);
    on_dtype(d->dtype, [&](auto T) {
      using E = decltype(T);
      hipLaunchKernelGGL((region_stats_fwd_kernel<E>), dim3((unsigned)rs_tiles(sh)), b, 0, s, sh, tab, (const E*)x,
                         (double*)workspace);
    });
    THZ_LAUNCH_CHECK();
    kt.stop();
  }
  KernelTimer kf("region_stats_finish", s);
  hipLaunchKernelGGL(region_stats_finish_kernel, dim3((unsigned)(sh.N * (sh.K + 1))), b, 0, s, sh, tab,
                     (const double*)workspace, out);
  THZ_LAUNCH_CHECK();
  kf.stop();
  return THZ_OK;
}

extern "C" int thz_region_stats_backward(const thz_region_stats_desc* d, const void* x, const double* G, void* grad,
                                         thz_stream_t stream) {
  const char* who = "thz_region_stats_backward";
  RsShape sh;
  RsTable tab;
  if (int e = rs_shape(who, d, &sh, &tab)) return e;
  if (rs_tiles(sh) == 0) return THZ_OK;
  const bool field = d->dtype == THZ_METRICS_C64 || d->dtype == THZ_METRICS_C128;
  if (field && !x) return fail(THZ_E_ARG, "%s: null field", who);
  if (!G || !grad) return fail(THZ_E_ARG, "%s: null pointer", who);
  if (misaligned(x, comp_bytes(d->dtype)) || misaligned(grad, comp_bytes(d->dtype)) || misaligned(G, sizeof(double)))
    return fail(THZ_E_ARG, "%s: array misaligned", who);
  sh.wide = rs_pitch16(sh, d->dtype) && all_aligned16({field ? x : nullptr, grad});
  hipStream_t s = (hipStream_t)stream;
  KernelTimer kt("region_stats_bwd", s);
  on_dtype(d->dtype, [&](auto T) {
    using E = decltype(T);
    hipLaunchKernelGGL((region_stats_bwd_kernel<E>), dim3((unsigned)rs_tiles(sh)), dim3(RS_THREADS), 0, s, sh, tab,
                       (const E*)x, G, (E*)grad);
  });
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}

extern "C" int thz_line_widths(const void* v, int dtype, long long L, int W, double level, double* out,
                               thz_stream_t stream) {
  const char* who = "thz_line_widths";
  if (dtype != THZ_METRICS_F32 && dtype != THZ_METRICS_F64) return fail(THZ_E_ARG, "%s: dtype %d (real lines)", who, dtype);
  if (L < 0 || W < 1) return fail(THZ_E_ARG, "%s: bad shape L = %lld, W = %d", who, L, W);
  if (!(level > 0.0 && level < 1.0)) return fail(THZ_E_ARG, "%s: level %g outside (0, 1)", who, level);
  const bool per_wave = W <= LW_WAVE_MAX;
  const long long blocks = per_wave ? (L + LW_WAVES - 1) / LW_WAVES : L;
  if (blocks > (1LL << 31) - 1) return fail(THZ_E_UNSUPPORTED, "%s: L = %lld lines beyond the grid's extent", who, L);
  if (L == 0) return THZ_OK;
  if (!v || !out) return fail(THZ_E_ARG, "%s: null pointer", who);
  if (misaligned(v, comp_bytes(dtype)) || misaligned(out, sizeof(double))) return fail(THZ_E_ARG, "%s: array misaligned", who);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g((unsigned)blocks), b(LW_THREADS);
  KernelTimer kt("line_widths", s);
  on_dtype(dtype, [&](auto T) {
    using E = decltype(T);
    if constexpr (std::is_same<E, float>::value || std::is_same<E, double>::value) {
      if (per_wave) hipLaunchKernelGGL((line_widths_kernel<E, true>), g, b, 0, s, (const E*)v, L, W, level, out);
      else hipLaunchKernelGGL((line_widths_kernel<E, false>), g, b, 0, s, (const E*)v, L, W, level, out);
    }
  });
  THZ_LAUNCH_CHECK();
  kt.stop();
  return THZ_OK;
}
