// jds_jpeg_inv.hpp — the tile core of the fused inverse for baseline JPEGs from
// elsewhere (jds_jpeg_inv.hip, k_jpeg_inv; DESIGN.md "Foreign files to
// pixels"): decoded coefficients in jds_decode_jpeg's layout -> RGB bytes with a
// quantisation table per component, T.81's ceil-sized block grids and cv2's
// general INTER_LINEAR taps, every operation fp64 in the reference's order
// (jds.codec.staged_inverse is the definition) with FP contraction off.
// Compiles for host and device: the GPU lanes, the host tile loop behind
// jds_selftest_jpeg_inverse and the stand-alone sanitizer program
// (tools/jpeg_inv_host_san.cpp) run this same code.  No HIP types here.
//
// One tile is JI_TH x JI_TW output pixels in every mode.  Eight lanes own a
// block: lane v transforms column v into the transpose buffer, then row v out of
// it (jds_inv_exact.hpp's idct_col / idct_row, restated without device
// intrinsics: the integer product and x/16 + 128 are exact either way).  With
// subsampled chroma a tile first transforms every chroma block its taps reach
// into a window of chroma samples (jpeg_inv_window), then its luma blocks, whose
// row pass upsamples, converts and stores 8 pixels.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "jds.h"
#include "jds_dct8.hpp"

#pragma clang fp contract(off)

#ifndef JDS_HDI
#ifdef __HIPCC__
#define JDS_HDI __host__ __device__ __forceinline__
#else
#define JDS_HDI inline
#endif
#endif

namespace jds {

constexpr int JI_TH = 32, JI_TW = 128;  // output pixels per tile
constexpr int JI_NT = 512;              // lanes per tile
constexpr int JI_NB = JI_NT / 8;        // blocks per round: the tile's 4 x 16 luma blocks are one round
constexpr int JI_MS = 72;               // doubles per block in the transpose buffer (jds_inv_common.hpp MS)
static_assert(JI_TH % 16 == 0 && JI_TW % 16 == 0 && (JI_TH / 8) * (JI_TW / 8) == JI_NB, "tile");

// The chroma window of a subsampled axis: a tile of T pixels reads at most
// T/2 + 2 samples (the taps of its first and last pixel are at most
// ceil((T - 1) * scale) + 1 apart and scale = ceil(n/2)/n <= (T + 1)/(2T) once
// the axis is longer than the tile); one more for the float rounding of the
// fraction.  Every launch checks the windows of its tiles against these
// (jinv_windows_fit), and tests/test_jpeg_rgb_cpu.py every size up to 200.
constexpr int JI_CAP_ROWS2 = JI_TH / 2 + 3, JI_CAP_COLS2 = JI_TW / 2 + 3;

template <int SS>
struct JInvCfg {
  static constexpr int SY = SS == JDS_SS_420 ? 2 : 1, SX = SS == JDS_SS_444 ? 1 : 2;
  static constexpr int CWR = SY == 2 ? JI_CAP_ROWS2 : JI_TH;  // window rows
  static constexpr int CWC = JI_CAP_COLS2;                    // window columns
  // row stride: 67 -> 70 doubles, 140 dwords = 12 mod 64 banks, so the two
  // window rows a 16-lane group reads (8 pixel rows = 4 or 5 chroma rows) start
  // on different banks (as k_inv2's 66 -> 70)
  static constexpr int CWS = CWC + 3;
  static constexpr int CWN = SX == 2 ? CWR * CWS : 1;  // 4:4:4 has no window
};

// Grayscale (one component, DESIGN.md "Grayscale files"): no chroma at all, so
// no window on either axis; the tile core below has a path of its own
// (jinv_gray_*), which never touches planes 1 and 2.
template <>
struct JInvCfg<JDS_SS_GRAY> {
  static constexpr int SY = 1, SX = 1;
  static constexpr int CWR = JI_TH, CWC = JI_CAP_COLS2, CWS = CWC + 3, CWN = 0;
};
constexpr int JI_MODES = 4;  // JDS_SS_444, _422, _420, _GRAY: one batch launch per mode present

// What a launch needs: passed by value as the kernel argument (no upload).
struct JInvArgs {
  int H, W, ss;
  int gr[3], gc[3];     // T.81 block grid per component (rows, columns); grayscale: zero for 1 and 2
  int ph, pw;           // chroma plane: ceil(H * Vc / Vmax) x ceil(W * Hc / Hmax); grayscale: 0 x 0
  int tiles_y, tiles_x;
  long long off[3];     // component offsets in the coefficient array
  double sy, sx;        // cv2's scale 1.0 / (dst / src) per axis
  int q[3][64];         // integer tables in [1, 255], row-major
};

JDS_HDI int jinv_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cv2 INTER_LINEAR (resizeGeneric, 64F) on one axis at destination index d:
// samples i0, i1 of an n-sample axis and the fraction f (weights 1.f - f and
// f).  Rows are clamped and keep their weights; in x a tap left of the plane is
// (0, f = 0) and one at or past the last sample is (n - 1, f = 0), where cv2
// copies S[sx] * 1: with f = 0 and i1 = i0 the two-tap form gives the same bits
// (samples are finite and >= 0).  oracle/cpu_ref.py:_linear_tab, k_gen_px.
struct JTap {
  int i0, i1;
  float f;
};
JDS_HDI JTap jinv_tap(int d, double scale, int n, bool xaxis) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)__builtin_floorf(f);
  f -= (float)s;
  if (xaxis) {
    if (s < 0) {
      s = 0;
      f = 0.f;
    }
    if (s >= n - 1) {
      s = n - 1;
      f = 0.f;
    }
  }
  JTap t;
  t.i0 = jinv_clamp(s, 0, n - 1);
  t.i1 = jinv_clamp(s + 1, 0, n - 1);
  t.f = f;
  return t;
}

// The samples of an n-sample chroma axis that destination indices d0..d1 read:
// [*origin, *origin + *extent).  Both tap indices are monotone in d, so the
// formula at the two ends bounds everything between; no ratio is assumed.
JDS_HDI void jpeg_inv_window(int d0, int d1, double scale, int n, bool xaxis, int* origin, int* extent) {
  const int lo = jinv_tap(d0, scale, n, xaxis).i0, hi = jinv_tap(d1, scale, n, xaxis).i1;
  *origin = lo;
  *extent = hi - lo + 1;
}

struct JWin {
  int Y0, X0, y1, x1;    // the tile's first and last pixel row / column inside H x W
  int wy0, eh, wx0, ew;  // chroma window: origin and extent in samples
  int cby0, ncbr, cbx0, ncbc;  // the chroma blocks that hold it
};

template <int SS>
JDS_HDI JWin jinv_tile_window(const JInvArgs& a, int ty, int tx) {
  using C = JInvCfg<SS>;
  JWin w;
  w.Y0 = ty * JI_TH;
  w.X0 = tx * JI_TW;
  w.y1 = (w.Y0 + JI_TH < a.H ? w.Y0 + JI_TH : a.H) - 1;
  w.x1 = (w.X0 + JI_TW < a.W ? w.X0 + JI_TW : a.W) - 1;
  w.wy0 = w.Y0;
  w.eh = w.y1 - w.Y0 + 1;
  w.wx0 = w.ew = 0;
  if (C::SY == 2) jpeg_inv_window(w.Y0, w.y1, a.sy, a.ph, false, &w.wy0, &w.eh);
  if (C::SX == 2) jpeg_inv_window(w.X0, w.x1, a.sx, a.pw, true, &w.wx0, &w.ew);
  w.cby0 = w.wy0 / 8;
  w.ncbr = (w.wy0 + w.eh - 1) / 8 - w.cby0 + 1;
  w.cbx0 = w.wx0 / 8;
  w.ncbc = C::SX == 2 ? (w.wx0 + w.ew - 1) / 8 - w.cbx0 + 1 : 0;
  return w;
}

// Every tile row's and tile column's window fits the LDS arrays (the product of
// a row interval and a column interval, each a function of its axis alone).
template <int SS>
inline bool jinv_windows_fit(const JInvArgs& a) {
  using C = JInvCfg<SS>;
  if (C::SX == 1) return true;
  for (int ty = 0; ty < a.tiles_y; ++ty) {
    const JWin w = jinv_tile_window<SS>(a, ty, 0);
    if (w.eh < 1 || w.eh > C::CWR) return false;
  }
  for (int tx = 0; tx < a.tiles_x; ++tx) {
    const JWin w = jinv_tile_window<SS>(a, 0, tx);
    if (w.ew < 1 || w.ew > C::CWC) return false;
  }
  return true;
}

// Geometry and tables of a parsed file.  0, or -(1 + 64 c + i) for table entry
// i of component c outside integer [1, 255] (check_tables' rule), or -1000 for a
// geometry that is not T.81's for H x W (the coefficient array is indexed by it).
inline int jinv_args(const jds_jpeg_info* info, JInvArgs* a) {
  memset(a, 0, sizeof *a);
  const int ss = info->subsampling;
  if (info->H < 1 || info->W < 1 || info->H * info->W > (int64_t)1 << 28 || info->H > 0x7fffffff ||
      info->W > 0x7fffffff || (ss != JDS_SS_444 && ss != JDS_SS_422 && ss != JDS_SS_420 && ss != JDS_SS_GRAY))
    return -1000;
  if (ss == JDS_SS_GRAY) {  // component 0 alone: the rest of the info is not read and the record keeps zeros
    a->H = (int)info->H;
    a->W = (int)info->W;
    a->ss = ss;
    a->gr[0] = (a->H + 7) / 8;
    a->gc[0] = (a->W + 7) / 8;
    if (info->grid_rows[0] != a->gr[0] || info->grid_cols[0] != a->gc[0]) return -1000;
    for (int i = 0; i < 64; ++i) {
      const double q = info->qtable[0][i];
      if (!(q >= 1.0 && q <= 255.0) || q != (double)(int)q) return -(1 + i);
      a->q[0][i] = (int)q;
    }
    if (info->coeffs_needed != 64ll * a->gr[0] * a->gc[0]) return -1000;
    a->sy = a->sx = 1.0;
    a->tiles_y = (a->H + JI_TH - 1) / JI_TH;
    a->tiles_x = (a->W + JI_TW - 1) / JI_TW;
    return 0;
  }
  const int vmax = ss == JDS_SS_420 ? 2 : 1, hmax = ss == JDS_SS_444 ? 1 : 2;
  a->H = (int)info->H;
  a->W = (int)info->W;
  a->ss = ss;
  a->ph = (a->H + vmax - 1) / vmax;
  a->pw = (a->W + hmax - 1) / hmax;
  long long off = 0;
  for (int c = 0; c < 3; ++c) {
    const int h = c ? a->ph : a->H, w = c ? a->pw : a->W;
    a->gr[c] = (h + 7) / 8;
    a->gc[c] = (w + 7) / 8;
    if (info->grid_rows[c] != a->gr[c] || info->grid_cols[c] != a->gc[c]) return -1000;
    a->off[c] = off;
    off += 64ll * a->gr[c] * a->gc[c];
    for (int i = 0; i < 64; ++i) {
      const double q = info->qtable[c][i];
      if (!(q >= 1.0 && q <= 255.0) || q != (double)(int)q) return -(1 + 64 * c + i);
      a->q[c][i] = (int)q;
    }
  }
  if (info->coeffs_needed != off) return -1000;
  a->sy = 1.0 / ((double)a->H / (double)a->ph);
  a->sx = 1.0 / ((double)a->W / (double)a->pw);
  a->tiles_y = (a->H + JI_TH - 1) / JI_TH;
  a->tiles_x = (a->W + JI_TW - 1) / JI_TW;
  return 0;
}

// What one workgroup keeps in LDS (the host loop: on the stack).
template <int SS>
struct JShared {
  double mid[JI_NB * JI_MS];
  double cw[2][JInvCfg<SS>::CWN];
  int q[3 * 64];
  int xi0[JI_TW], xi1[JI_TW];  // column taps of the tile's pixels, relative to the window
  float xf[JI_TW];
};

// Grayscale: the transpose buffer and one table (36.25 KB).
template <>
struct JShared<JDS_SS_GRAY> {
  double mid[JI_NB * JI_MS];
  int q[64];
};

// jds_inv_common.hpp's tslot: the 16-B pair c/2 of row r sits at pair
// (c/2) ^ (r & 3), so neither the column writes nor the row reads of the 8
// blocks of a wave collide on LDS banks.
JDS_HDI int jinv_slot(int r, int c) { return r * 8 + ((((c >> 1) ^ (r & 3)) << 1) | (c & 1)); }

// Dequantise (an exact integer product: |coefficient| < 2^15, Q <= 255) and
// transform column v of a block, on 16x the reference's operands (idct_col).
JDS_HDI void jinv_col(const int16_t* blk, const int* q, int v, double* mid) {
  double c[8];
  for (int r = 0; r < 8; ++r) c[r] = (double)((int)blk[r * 8 + v] * q[r * 8 + v]);
  dct3_line(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
  for (int r = 0; r < 8; ++r) mid[jinv_slot(r, v)] = c[r];
}

// Row u: second pass, the exact 1/16, +128, clip (idct_row).
JDS_HDI void jinv_row(const double* mid, int u, double (&c)[8]) {
  for (int k = 0; k < 8; ++k) c[k] = mid[jinv_slot(u, k)];
  dct3_line(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
  for (int k = 0; k < 8; ++k) {
    const double s = c[k] * 0.0625 + 128.0;
    c[k] = s < 0.0 ? 0.0 : (s > 255.0 ? 255.0 : s);
  }
}

// Lane k of the tile: the column taps of pixel X0 + k (zeros past the image).
template <int SS>
JDS_HDI void jinv_xtap(JShared<SS>& sh, const JInvArgs& a, const JWin& w, int k) {
  using C = JInvCfg<SS>;
  int i0 = 0, i1 = 0;
  float f = 0.f;
  if (C::SX == 2 && w.X0 + k <= w.x1) {
    const JTap t = jinv_tap(w.X0 + k, a.sx, a.pw, true);
    i0 = jinv_clamp(t.i0 - w.wx0, 0, C::CWC - 1);
    i1 = jinv_clamp(t.i1 - w.wx0, 0, C::CWC - 1);
    f = t.f;
  }
  sh.xi0[k] = i0;
  sh.xi1[k] = i1;
  sh.xf[k] = f;
}

// Chroma task t of a tile: plane t / (blocks of the window), block t % .. in
// raster order of the window's blocks; its transpose slot is t % JI_NB.
struct JTask {
  int p, by, bx;
  bool ok;
};
JDS_HDI JTask jinv_chroma_task(const JInvArgs& a, const JWin& w, int t) {
  const int ncb = w.ncbr * w.ncbc;
  JTask k;
  k.p = t / ncb;
  const int b = t - k.p * ncb, i = b / w.ncbc;
  k.by = w.cby0 + i;
  k.bx = w.cbx0 + (b - i * w.ncbc);
  k.ok = k.p < 2 && k.by < a.gr[1] && k.bx < a.gc[1];
  return k;
}

template <int SS>
JDS_HDI void jinv_chroma_col(JShared<SS>& sh, const JInvArgs& a, const JWin& w, const int16_t* coeffs, int t, int v) {
  const JTask k = jinv_chroma_task(a, w, t);
  if (!k.ok) return;
  jinv_col(coeffs + a.off[1 + k.p] + ((long long)k.by * a.gc[1] + k.bx) * 64, sh.q + 64 * (1 + k.p), v,
           sh.mid + (t % JI_NB) * JI_MS);
}

// Row u of the block goes into the window where the window holds it (a block
// at the window's edge contributes only some rows and columns).
template <int SS>
JDS_HDI void jinv_chroma_row(JShared<SS>& sh, const JInvArgs& a, const JWin& w, int t, int u) {
  using C = JInvCfg<SS>;
  const JTask k = jinv_chroma_task(a, w, t);
  const int wr = k.by * 8 + u - w.wy0;
  if (!k.ok || wr < 0 || wr >= w.eh || wr >= C::CWR) return;
  double c[8];
  jinv_row(sh.mid + (t % JI_NB) * JI_MS, u, c);
  double* row = &sh.cw[k.p][C::SX == 2 ? wr * C::CWS : 0];
  const int wc0 = k.bx * 8 - w.wx0;
  for (int j = 0; j < 8; ++j)
    if (wc0 + j >= 0 && wc0 + j < w.ew && wc0 + j < C::CWC) row[wc0 + j] = c[j];
}

// Luma block lb of the tile (raster order, JI_TW / 8 per row).
JDS_HDI bool jinv_luma_block(const JInvArgs& a, const JWin& w, int lb, int* by, int* bx) {
  const int bi = lb / (JI_TW / 8);
  *by = w.Y0 / 8 + bi;
  *bx = w.X0 / 8 + (lb - bi * (JI_TW / 8));
  return *by < a.gr[0] && *bx < a.gc[0] && *by * 8 <= w.y1 && *bx * 8 <= w.x1;
}

// One plane's upsampled chroma at the 8 pixels from column x0 of row y
// (gen_upsample's expressions: the horizontal taps on two window rows, then the
// vertical blend; without vertical subsampling cv2's second row has weight 0
// and the first row's value stands).
template <int SS>
JDS_HDI void jinv_chroma_up(const JShared<SS>& sh, const JInvArgs& a, const JWin& w, int y, int x0, int p,
                            double (&Cv)[8]) {
  using C = JInvCfg<SS>;
  int r0 = jinv_clamp(y - w.wy0, 0, C::CWR - 1), r1 = r0;
  double b0 = 1.0, b1 = 0.0;
  if (C::SY == 2) {
    const JTap t = jinv_tap(y, a.sy, a.ph, false);
    r0 = jinv_clamp(t.i0 - w.wy0, 0, C::CWR - 1);
    r1 = jinv_clamp(t.i1 - w.wy0, 0, C::CWR - 1);
    b0 = (double)(1.f - t.f);
    b1 = (double)t.f;
  }
  const double* s0 = &sh.cw[p][C::SX == 2 ? r0 * C::CWS : 0];
  const double* s1 = &sh.cw[p][C::SX == 2 ? r1 * C::CWS : 0];
  for (int k = 0; k < 8; ++k) {
    const int kk = x0 - w.X0 + k;
    const int i0 = sh.xi0[kk], i1 = sh.xi1[kk];
    const float f = sh.xf[kk];
    const double a0 = (double)(1.f - f), a1 = (double)f;
    const double h0 = s0[i0] * a0 + s0[i1] * a1;
    if (C::SY == 2) {
      const double h1 = s1[i0] * a0 + s1[i1] * a1;
      Cv[k] = h0 * b0 + h1 * b1;
    } else {
      Cv[k] = h0;
    }
  }
}

// NumPy's colour expressions left to right (k_gen_px), clip, truncate, and the
// first nx of 8 pixels as packed bytes at o.
JDS_HDI void jinv_colour_store(const double (&Yv)[8], const double (&Cb)[8], const double (&Cr)[8], uint8_t* o,
                               int nx) {
  uint32_t pk[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (int k = 0; k < 8; ++k) {
    double R = Yv[k] + 1.402 * (Cr[k] - 128.0);
    double G = Yv[k] - 0.344136 * (Cb[k] - 128.0) - 0.714136 * (Cr[k] - 128.0);
    double B = Yv[k] + 1.772 * (Cb[k] - 128.0);
    R = R < 0.0 ? 0.0 : (R > 255.0 ? 255.0 : R);
    G = G < 0.0 ? 0.0 : (G > 255.0 ? 255.0 : G);
    B = B < 0.0 ? 0.0 : (B > 255.0 ? 255.0 : B);
    const int b = 3 * k;
    pk[b >> 2] |= (uint32_t)(int)R << (8 * (b & 3));
    pk[(b + 1) >> 2] |= (uint32_t)(int)G << (8 * ((b + 1) & 3));
    pk[(b + 2) >> 2] |= (uint32_t)(int)B << (8 * ((b + 2) & 3));
  }
  if (nx == 8 && (((uintptr_t)o) & 7u) == 0) {
    uint8_t* o8 = (uint8_t*)__builtin_assume_aligned(o, 8);
    for (int i = 0; i < 3; ++i) {
      const uint64_t v = (uint64_t)pk[2 * i] | ((uint64_t)pk[2 * i + 1] << 32);
      __builtin_memcpy(o8 + 8 * i, &v, 8);
    }
  } else {
    for (int b = 0; b < 24; ++b)
      if (b < 3 * nx) o[b] = (uint8_t)(pk[b >> 2] >> (8 * (b & 3)));
  }
}

// Grayscale: (Y, Y, Y) per pixel in jinv_colour_store's packing.  With
// Cb = Cr = 128 its expressions are Y + c * 0.0 = Y exactly and Y is already
// clipped (jinv_row), so the byte is the truncated sample in all three channels.
JDS_HDI void jinv_gray_store(const double (&Yv)[8], uint8_t* o, int nx) {
  uint32_t pk[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (int k = 0; k < 8; ++k) {
    const uint32_t y = (uint32_t)(int)Yv[k];
    for (int b = 3 * k; b < 3 * k + 3; ++b) pk[b >> 2] |= y << (8 * (b & 3));
  }
  if (nx == 8 && (((uintptr_t)o) & 7u) == 0) {
    uint8_t* o8 = (uint8_t*)__builtin_assume_aligned(o, 8);
    for (int i = 0; i < 3; ++i) {
      const uint64_t v = (uint64_t)pk[2 * i] | ((uint64_t)pk[2 * i + 1] << 32);
      __builtin_memcpy(o8 + 8 * i, &v, 8);
    }
  } else {
    for (int b = 0; b < 24; ++b)
      if (b < 3 * nx) o[b] = (uint8_t)(pk[b >> 2] >> (8 * (b & 3)));
  }
}

// A grayscale tile on the host: its luma blocks and nothing else.
inline void jinv_host_tile_gray(JShared<JDS_SS_GRAY>& sh, const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, int ty,
                                int tx) {
  const JWin w = jinv_tile_window<JDS_SS_GRAY>(a, ty, tx);
  for (int lb = 0; lb < JI_NB; ++lb) {
    int by, bx;
    if (!jinv_luma_block(a, w, lb, &by, &bx)) continue;
    double* mid = sh.mid + lb * JI_MS;
    const long long boff = ((long long)by * a.gc[0] + bx) * 64;
    double Yv[8];
    for (int v = 0; v < 8; ++v) jinv_col(coeffs + boff, sh.q, v, mid);
    for (int u = 0; u < 8; ++u) {
      const int y = by * 8 + u, x0 = bx * 8;
      if (y > w.y1) continue;
      jinv_row(mid, u, Yv);
      const int nx = w.x1 + 1 - x0 < 8 ? w.x1 + 1 - x0 : 8;
      jinv_gray_store(Yv, rgb + ((size_t)y * a.W + x0) * 3, nx);
    }
  }
}

// One tile on the host: the kernel's steps with loops in place of lanes and of
// the barriers between them.  sh.q holds the image's tables.  No GPU.
template <int SS>
inline void jinv_host_tile(JShared<SS>& sh, const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, int ty, int tx) {
  using C = JInvCfg<SS>;
  const JWin w = jinv_tile_window<SS>(a, ty, tx);
  for (int k = 0; k < JI_TW; ++k) jinv_xtap<SS>(sh, a, w, k);
  if (C::SX == 2)
    for (int t0 = 0; t0 < 2 * w.ncbr * w.ncbc; t0 += JI_NB) {
      for (int t = t0; t < t0 + JI_NB; ++t)
        for (int v = 0; v < 8; ++v) jinv_chroma_col<SS>(sh, a, w, coeffs, t, v);
      for (int t = t0; t < t0 + JI_NB; ++t)
        for (int u = 0; u < 8; ++u) jinv_chroma_row<SS>(sh, a, w, t, u);
    }
  for (int lb = 0; lb < JI_NB; ++lb) {
    int by, bx;
    if (!jinv_luma_block(a, w, lb, &by, &bx)) continue;
    double* mid = sh.mid + lb * JI_MS;
    const long long boff = ((long long)by * a.gc[0] + bx) * 64;
    double Yv[8][8], Cb[8][8], Cr[8][8];
    for (int v = 0; v < 8; ++v) jinv_col(coeffs + a.off[0] + boff, sh.q, v, mid);
    for (int u = 0; u < 8; ++u) jinv_row(mid, u, Yv[u]);
    if (C::SX == 1) {
      for (int v = 0; v < 8; ++v) jinv_col(coeffs + a.off[1] + boff, sh.q + 64, v, mid);
      for (int u = 0; u < 8; ++u) jinv_row(mid, u, Cb[u]);
      for (int v = 0; v < 8; ++v) jinv_col(coeffs + a.off[2] + boff, sh.q + 128, v, mid);
      for (int u = 0; u < 8; ++u) jinv_row(mid, u, Cr[u]);
    }
    for (int u = 0; u < 8; ++u) {
      const int y = by * 8 + u, x0 = bx * 8;
      if (y > w.y1) continue;
      if (C::SX == 2) {
        jinv_chroma_up<SS>(sh, a, w, y, x0, 0, Cb[u]);
        jinv_chroma_up<SS>(sh, a, w, y, x0, 1, Cr[u]);
      }
      const int nx = w.x1 + 1 - x0 < 8 ? w.x1 + 1 - x0 : 8;
      jinv_colour_store(Yv[u], Cb[u], Cr[u], rgb + ((size_t)y * a.W + x0) * 3, nx);
    }
  }
}

// The host tile loop of one image.
template <int SS>
inline void jinv_host_image(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb) {
  JShared<SS>* shp = new JShared<SS>();  // (zeroed: the lanes past the image's right edge read finite samples)
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < 64; ++i) shp->q[64 * c + i] = a.q[c][i];
  for (int ty = 0; ty < a.tiles_y; ++ty)
    for (int tx = 0; tx < a.tiles_x; ++tx) jinv_host_tile<SS>(*shp, a, coeffs, rgb, ty, tx);
  delete shp;
}

template <>
inline void jinv_host_image<JDS_SS_GRAY>(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb) {
  JShared<JDS_SS_GRAY>* shp = new JShared<JDS_SS_GRAY>();
  for (int i = 0; i < 64; ++i) shp->q[i] = a.q[0][i];
  for (int ty = 0; ty < a.tiles_y; ++ty)
    for (int tx = 0; tx < a.tiles_x; ++tx) jinv_host_tile_gray(*shp, a, coeffs, rgb, ty, tx);
  delete shp;
}

// ------------------------------------------------------------- batches --
//
// k_jpeg_inv_batch (DESIGN.md "Batches of foreign files"): one launch per
// subsampling mode over the tiles of that mode's images.  The per-image records
// live in a device array; a launch has a map of its images -- (first tile,
// record) per image in batch order, closed by a sentinel holding the launch's
// tile count -- and a workgroup finds its image by a binary search over the
// first tiles (jinv_find: scalar loads, log2(images) steps).

// One image of a batch: its launch arguments, where its coefficients and its
// pixels start in the batch's buffers, and its status word (an image whose
// decode set a bit there is not inverted: its pixels are zero).
struct JInvRec {
  JInvArgs a;
  long long coef_off;  // entries from the batch's coefficient base
  long long rgb_off;   // bytes from the batch's output base: a multiple of JI_RGB_ALIGN
  int st;              // index of its status word
  int pad_;
};
constexpr long long JI_RGB_ALIGN = 256;

// The layout step: image k of a batch (its arguments in r.a) goes behind the
// ones placed so far -- pixels at the next multiple of JI_RGB_ALIGN, coefficients
// end to end -- and gets status word k.
inline void jinv_batch_place(JInvRec& r, int k, long long coeffs_needed, long long* rgb_bytes, long long* coef_entries) {
  r.coef_off = *coef_entries;
  r.rgb_off = *rgb_bytes;
  r.st = k;
  *coef_entries += coeffs_needed;
  const long long nimg = (long long)r.a.H * r.a.W * 3;
  *rgb_bytes += (nimg + JI_RGB_ALIGN - 1) / JI_RGB_ALIGN * JI_RGB_ALIGN;
}

struct JInvMap {
  int tile0;  // the image's first tile in its mode's launch (sentinel: the launch's tiles)
  int rec;    // its record
};

// The map entry of tile t: the last i in [0, n) with map[i].tile0 <= t (n >= 1
// images, map[0].tile0 == 0, t < map[n].tile0; an image has at least one tile).
JDS_HDI int jinv_find(const JInvMap* map, int n, int t) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (map[mid].tile0 <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// The host model of the batch launches: the same map walk and the same records
// through jinv_host_tile; a flagged image's tiles are zero-filled.
template <int SS>
inline void jinv_host_batch_mode(const JInvRec* recs, const JInvMap* map, int nmap, const uint32_t* status,
                                 const int16_t* coeffs, uint8_t* rgb) {
  if (nmap < 1) return;
  JShared<SS>* shp = new JShared<SS>();
  for (int t = 0; t < map[nmap].tile0; ++t) {
    const int mi = jinv_find(map, nmap, t);
    const JInvRec& r = recs[map[mi].rec];
    const JInvArgs& a = r.a;
    const int lt = t - map[mi].tile0, ty = lt / a.tiles_x, tx = lt - ty * a.tiles_x;
    uint8_t* o = rgb + r.rgb_off;
    if (status[r.st]) {
      const JWin w = jinv_tile_window<SS>(a, ty, tx);
      for (int y = w.Y0; y <= w.y1; ++y) memset(o + ((size_t)y * a.W + w.X0) * 3, 0, 3 * (size_t)(w.x1 - w.X0 + 1));
      continue;
    }
    if constexpr (SS == JDS_SS_GRAY) {
      for (int i = 0; i < 64; ++i) shp->q[i] = a.q[0][i];
      jinv_host_tile_gray(*shp, a, coeffs + r.coef_off, o, ty, tx);
    } else {
      for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 64; ++i) shp->q[64 * c + i] = a.q[c][i];
      jinv_host_tile<SS>(*shp, a, coeffs + r.coef_off, o, ty, tx);
    }
  }
  delete shp;
}

// map[m] / nmap[m]: the launch of subsampling code m (JDS_SS_444, _422, _420, _GRAY = 0, 1, 2, 3).
inline void jpeg_inv_batch_host(const JInvRec* recs, const JInvMap* const map[JI_MODES], const int nmap[JI_MODES],
                                const uint32_t* status, const int16_t* coeffs, uint8_t* rgb) {
  jinv_host_batch_mode<JDS_SS_444>(recs, map[JDS_SS_444], nmap[JDS_SS_444], status, coeffs, rgb);
  jinv_host_batch_mode<JDS_SS_422>(recs, map[JDS_SS_422], nmap[JDS_SS_422], status, coeffs, rgb);
  jinv_host_batch_mode<JDS_SS_420>(recs, map[JDS_SS_420], nmap[JDS_SS_420], status, coeffs, rgb);
  jinv_host_batch_mode<JDS_SS_GRAY>(recs, map[JDS_SS_GRAY], nmap[JDS_SS_GRAY], status, coeffs, rgb);
}

// The maps of a batch from its records (in batch order).  false: a mode's tiles
// exceed what a grid and a 32-bit tile index take.
inline bool jinv_batch_maps(const JInvRec* recs, int nrec, std::vector<JInvMap> (&map)[JI_MODES]) {
  long long tiles[JI_MODES] = {0, 0, 0, 0};
  for (int m = 0; m < JI_MODES; ++m) map[m].clear();
  for (int i = 0; i < nrec; ++i) {
    const int m = recs[i].a.ss;
    map[m].push_back(JInvMap{(int)tiles[m], i});
    tiles[m] += (long long)recs[i].a.tiles_y * recs[i].a.tiles_x;
    if (tiles[m] > 0x7fffffffll) return false;
  }
  for (int m = 0; m < JI_MODES; ++m) map[m].push_back(JInvMap{(int)tiles[m], -1});
  return true;
}

}  // namespace jds
