// jds_jpeg_ljs.hpp — the tile core of the scaled libjpeg rendering
// (jds_jpeg_ljs.hip, k_jpeg_ljs; DESIGN.md "Scaled libjpeg rendering"): decoded
// coefficients in jds_decode_jpeg's layout -> the RGB bytes libjpeg gives with
// scale_num / scale_denom = 1/2, 1/4 or 1/8 (Pillow's Image.draft): jidctred's
// reduced inverses, a larger inverse for subsampled chroma than for luma where
// libjpeg picks one, h2v1 upsampling where one is left, jdcolor's conversion
// (tests/libjpeg_scaled_ref.py is the definition).  Arithmetic, transpose
// slotting, packing and colour are jds_jpeg_ljt.hpp's: 32-bit integers modulo
// 2^32, full 32-bit multiplies in both passes.  Compiles for host and device:
// the GPU lanes, the host tile loop behind jds_selftest_jpeg_render_scaled and
// tools/jpeg_ljs_san.cpp run this same code.
//
// A tile is the full-scale tile's 4 x 16 luma blocks, so JI_TH / D x JI_TW / D
// output pixels with the same tile grid, and eight lanes own a block: lane v
// does column v of the first pass where the reduced inverse reads it, lanes
// u < M (M = 8 / D) a row each.  Subsampled chroma goes first into a window of
// samples (4:2:0: one per pixel, no halo; 4:2:2: half as many and one of halo
// left and right, the plane's edge sample repeated outside it).  The pixels go
// to a staging tile in LDS and leave it four at a time: three dwords where the
// address allows, bytes otherwise.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "jds.h"
#include "jds_jpeg_ljt.hpp"

namespace jds {

constexpr bool ls_denom_ok(int d) { return d == 1 || d == 2 || d == 4 || d == 8; }
constexpr int ls_denom_index(int d) { return d == 2 ? 0 : d == 4 ? 1 : 2; }  // of 2, 4, 8
constexpr int LS_ND = 3;                                                      // scaled denominators

// libjpeg's DCT_scaled_size of a 1 x 1 component under hmax x vmax luma with
// min_DCT_scaled_size m: doubled while the luma's extent stays a multiple of it.
constexpr int ls_chroma_size(int m, int hmax, int vmax) {
  int s = m;
  while (s < 8 && (hmax * m) % (2 * s) == 0 && (vmax * m) % (2 * s) == 0) s *= 2;
  return s;
}

template <int SS, int D>
struct LsCfg {
  static_assert(D == 2 || D == 4 || D == 8, "scale_denom");
  static constexpr int M = 8 / D;  // the luma inverse's size: libjpeg's min_DCT_scaled_size
  static constexpr int HMAX = (SS == JDS_SS_422 || SS == JDS_SS_420) ? 2 : 1, VMAX = SS == JDS_SS_420 ? 2 : 1;
  static constexpr int S = ls_chroma_size(M, HMAX, VMAX);  // the chroma inverse's size
  static constexpr int UX = HMAX * M / S, UY = VMAX * M / S;  // what is left to upsample
  static_assert(UY == 1 && (UX == 1 || UX == 2), "h2v2 does not occur at 1/2, 1/4, 1/8");
  static constexpr int TH = JI_TH / D, TW = JI_TW / D;  // output pixels per tile
  static constexpr bool WIN = HMAX == 2;                // chroma through a window
  static constexpr int CWC = UX == 2 ? TW / 2 + 2 : TW;
  static constexpr int WS = CWC + 4;  // int16 per window row (4:2:0 at 1/2: 34 dwords, rows 34 banks apart)
  static constexpr int CWN = WIN ? TH * WS : 4;
  static constexpr int NCH = TW / 4;  // 4-pixel chunks per staged row
};

template <int SS, int D>
struct LsShared {
  int32_t mid[JI_NB * LJ_MS];
  alignas(8) int16_t cw[2][LsCfg<SS, D>::CWN];
  alignas(8) uint8_t st[LsCfg<SS, D>::TH * LsCfg<SS, D>::TW * 3];
  int q[3 * 64];
};

// Output and (scaled, cropped) chroma plane of an image.
struct LsGeo {
  int OH, OW, ph, pw;
};
template <int SS, int D>
JDS_HDI LsGeo ls_geo(const JInvArgs& a) {
  using C = LsCfg<SS, D>;
  LsGeo g;
  g.OH = (a.H + D - 1) / D;
  g.OW = (a.W + D - 1) / D;
  g.ph = (int)(((long long)a.H * C::S + 8 * C::VMAX - 1) / (8 * C::VMAX));
  g.pw = (int)(((long long)a.W * C::S + 8 * C::HMAX - 1) / (8 * C::HMAX));
  return g;
}

// jidctred's 4-point pass on in[0..3, 5..7], outputs DESCALEd by N.
template <int N>
JDS_HDI void ls_idct4(const int32_t (&in)[8], int32_t (&out)[4]) {
  const uint32_t i0 = (uint32_t)in[0], i1 = (uint32_t)in[1], i2 = (uint32_t)in[2], i3 = (uint32_t)in[3],
                 i5 = (uint32_t)in[5], i6 = (uint32_t)in[6], i7 = (uint32_t)in[7];
  const uint32_t t0 = i0 << 14, t2 = i2 * 15137u - i6 * 6270u, t10 = t0 + t2, t12 = t0 - t2;
  const uint32_t a = i5 * 11893u + i1 * 8697u - i7 * 1730u - i3 * 17799u;
  const uint32_t b = i3 * 7373u + i1 * 20995u - i7 * 4176u - i5 * 4926u;
  out[0] = lj_descale(t10 + b, N);
  out[1] = lj_descale(t12 + a, N);
  out[2] = lj_descale(t12 - a, N);
  out[3] = lj_descale(t10 - b, N);
}

// jidctred's 2-point pass on in[0, 1, 3, 5, 7].
template <int N>
JDS_HDI void ls_idct2(const int32_t (&in)[8], int32_t (&out)[2]) {
  const uint32_t i0 = (uint32_t)in[0], i1 = (uint32_t)in[1], i3 = (uint32_t)in[3], i5 = (uint32_t)in[5],
                 i7 = (uint32_t)in[7];
  const uint32_t t10 = i0 << 15, t = i5 * 6967u + i1 * 29692u - i7 * 5906u - i3 * 10426u;
  out[0] = lj_descale(t10 + t, N);
  out[1] = lj_descale(t10 - t, N);
}

// The lines an N-point pass reads.
template <int N>
JDS_HDI bool ls_line_used(int k) {
  return N == 8 ? true : N == 4 ? k != 4 : N == 2 ? (k == 0 || (k & 1)) : k == 0;
}

// Column v of a block through the N-point first pass into rows 0..N-1 of the
// transpose buffer (N == 1: the dequantised DC alone).
template <int N>
JDS_HDI void ls_col(const int16_t* blk, const int* q, int v, int32_t* mid) {
  if constexpr (N == 8) {
    lj_col(blk, q, v, mid);
  } else if constexpr (N == 1) {
    if (v == 0) mid[0] = lj_mul24((int)blk[0], q[0]);
  } else {
    if (!ls_line_used<N>(v)) return;
    int32_t c[8], o[N];
    for (int r = 0; r < 8; ++r) c[r] = ls_line_used<N>(r) ? lj_mul24((int)blk[r * 8 + v], q[r * 8 + v]) : 0;
    if constexpr (N == 4)
      ls_idct4<12>(c, o);
    else
      ls_idct2<13>(c, o);
    for (int r = 0; r < N; ++r) mid[lj_slot(r, v)] = o[r];
  }
}

// Row u < N: the second pass, + 128, clamp.
template <int N>
JDS_HDI void ls_row(const int32_t* mid, int u, int (&c)[N]) {
  if constexpr (N == 8) {
    lj_row(mid, u, c);
  } else if constexpr (N == 1) {
    c[0] = jinv_clamp((int32_t)((uint32_t)lj_descale((uint32_t)mid[0], 3) + 128u), 0, 255);
  } else {
    int32_t in[8], o[N];
    for (int k = 0; k < 8; ++k) in[k] = ls_line_used<N>(k) ? mid[lj_slot(u, k)] : 0;
    if constexpr (N == 4)
      ls_idct4<19>(in, o);
    else
      ls_idct2<20>(in, o);
    for (int k = 0; k < N; ++k) c[k] = jinv_clamp((int32_t)((uint32_t)o[k] + 128u), 0, 255);
  }
}

// The tile's output pixels (Y0, X0, y1, x1), its window's origin in samples of
// the scaled chroma plane (4:2:2: one left of the tile's first, -1 at the
// image's edge) and the chroma blocks, S x S samples each, that hold the
// window's samples inside the plane.
template <int SS, int D>
JDS_HDI JWin ls_tile_window(const LsGeo& g, int ty, int tx) {
  using C = LsCfg<SS, D>;
  JWin w;
  w.Y0 = ty * C::TH;
  w.X0 = tx * C::TW;
  w.y1 = (w.Y0 + C::TH < g.OH ? w.Y0 + C::TH : g.OH) - 1;
  w.x1 = (w.X0 + C::TW < g.OW ? w.X0 + C::TW : g.OW) - 1;
  w.wy0 = w.Y0;
  w.eh = C::TH;
  w.wx0 = C::UX == 2 ? w.X0 / 2 - 1 : w.X0;
  w.ew = C::CWC;
  w.cby0 = w.ncbr = w.cbx0 = w.ncbc = 0;
  if (C::WIN) {
    const int yhi = w.wy0 + C::TH - 1 < g.ph - 1 ? w.wy0 + C::TH - 1 : g.ph - 1;
    const int xlo = w.wx0 < 0 ? 0 : w.wx0, xhi = w.wx0 + C::CWC - 1 < g.pw - 1 ? w.wx0 + C::CWC - 1 : g.pw - 1;
    w.cby0 = w.wy0 / C::S;
    w.ncbr = yhi / C::S - w.cby0 + 1;
    w.cbx0 = xlo / C::S;
    w.ncbc = xhi / C::S - w.cbx0 + 1;
  }
  return w;
}

template <int SS, int D>
JDS_HDI void ls_chroma_col(LsShared<SS, D>& sh, const JInvArgs& a, const JWin& w, const int16_t* coeffs, int t, int v) {
  const JTask k = jinv_chroma_task(a, w, t);
  if (!k.ok) return;
  ls_col<LsCfg<SS, D>::S>(coeffs + a.off[1 + k.p] + ((long long)k.by * a.gc[1] + k.bx) * 64, sh.q + 64 * (1 + k.p), v,
                          sh.mid + (t % JI_NB) * LJ_MS);
}

// Row u of the block into the window: only samples of the cropped plane; with
// upsampling left, an edge sample also one place outside the plane.
template <int SS, int D>
JDS_HDI void ls_chroma_row(LsShared<SS, D>& sh, const JInvArgs& a, const LsGeo& g, const JWin& w, int t, int u) {
  using C = LsCfg<SS, D>;
  if (u >= C::S) return;
  const JTask k = jinv_chroma_task(a, w, t);
  const int cy = k.by * C::S + u, wr = cy - w.wy0;
  if (!k.ok || cy >= g.ph || wr < 0 || wr >= C::TH) return;
  int c[C::S];
  ls_row<C::S>(sh.mid + (t % JI_NB) * LJ_MS, u, c);
  int16_t* row = &sh.cw[k.p][C::WIN ? wr * C::WS : 0];
  for (int j = 0; j < C::S; ++j) {
    const int cx = k.bx * C::S + j, wc = cx - w.wx0;
    if (cx >= g.pw) break;
    if (wc >= 0 && wc < C::CWC) row[wc] = (int16_t)c[j];
    if (C::UX == 2) {
      if (cx == 0 && wc >= 1 && wc - 1 < C::CWC) row[wc - 1] = (int16_t)c[j];
      if (cx == g.pw - 1 && wc + 1 >= 0 && wc + 1 < C::CWC) row[wc + 1] = (int16_t)c[j];
    }
  }
}

// One plane's chroma at the M pixels from column x0 of row y: the sample under
// the pixel (4:2:0), or jdsample's h2v1 -- fancy taps when M > 1 and the plane
// is more than two samples wide, replication otherwise (4:2:2).
template <int SS, int D>
JDS_HDI void ls_chroma_px(const LsShared<SS, D>& sh, const LsGeo& g, const JWin& w, int y, int x0, int p,
                          int (&Cv)[LsCfg<SS, D>::M]) {
  using C = LsCfg<SS, D>;
  const int16_t* row = &sh.cw[p][C::WIN ? (y - w.wy0) * C::WS : 0];
  if (C::UX == 1) {
    for (int k = 0; k < C::M; ++k) Cv[k] = row[x0 - w.wx0 + k];
    return;
  }
  const bool fancy = C::M > 1 && g.pw > 2;
  for (int k = 0; k < C::M; ++k) {
    const int x = x0 + k, wc = (x >> 1) - w.wx0, s = row[wc];
    Cv[k] = !fancy ? s : (x & 1) ? (3 * s + row[wc + 1] + 2) >> 2 : (3 * s + row[wc - 1] + 1) >> 2;
  }
}

// Luma block lb of the tile; every block of the grid holds output pixels.
JDS_HDI bool ls_luma_block(const JInvArgs& a, int ty, int tx, int lb, int* by, int* bx) {
  const int bi = lb / (JI_TW / 8);
  *by = ty * (JI_TH / 8) + bi;
  *bx = tx * (JI_TW / 8) + (lb - bi * (JI_TW / 8));
  return *by < a.gr[0] && *bx < a.gc[0];
}

// M pixels of row y from column x0 into the staging tile: jdcolor, packed.
template <int SS, int D>
JDS_HDI void ls_emit(LsShared<SS, D>& sh, const JWin& w, int y, int x0, const int (&Yv)[LsCfg<SS, D>::M],
                     const int (&Cb)[LsCfg<SS, D>::M], const int (&Cr)[LsCfg<SS, D>::M]) {
  using C = LsCfg<SS, D>;
  int ch[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < C::M; ++k) {
    if (SS == JDS_SS_GRAY) {
      ch[3 * k] = ch[3 * k + 1] = ch[3 * k + 2] = Yv[k];
    } else {
      const int cb = Cb[k] - 128, cr = Cr[k] - 128;
      ch[3 * k] = Yv[k] + ((lj_mul24(91881, cr) + 32768) >> 16);
      ch[3 * k + 1] = Yv[k] + ((lj_mul24(-22554, cb) + lj_mul24(-46802, cr) + 32768) >> 16);
      ch[3 * k + 2] = Yv[k] + ((lj_mul24(116130, cb) + 32768) >> 16);
    }
  }
  uint8_t* o = &sh.st[((y - w.Y0) * C::TW + (x0 - w.X0)) * 3];
  const uint32_t p0 = lj_pack4(ch[0], ch[1], ch[2], ch[3]);
  if constexpr (C::M == 4) {
    const uint32_t pk[3] = {p0, lj_pack4(ch[4], ch[5], ch[6], ch[7]), lj_pack4(ch[8], ch[9], ch[10], ch[11])};
    __builtin_memcpy(__builtin_assume_aligned(o, 4), pk, 12);
  } else if constexpr (C::M == 2) {
    const uint32_t p1 = lj_pack4(ch[4], ch[5], 0, 0);
    const uint16_t h[3] = {(uint16_t)p0, (uint16_t)(p0 >> 16), (uint16_t)p1};
    __builtin_memcpy(__builtin_assume_aligned(o, 2), h, 6);
  } else {
    o[0] = (uint8_t)p0;
    o[1] = (uint8_t)(p0 >> 8);
    o[2] = (uint8_t)(p0 >> 16);
  }
}

// Lane i of the store: four staged pixels of one tile row to the image, as
// three dwords where the address is a multiple of 4, bytes otherwise.
template <int SS, int D>
JDS_HDI void ls_store(const LsShared<SS, D>& sh, const LsGeo& g, const JWin& w, uint8_t* rgb, int i) {
  using C = LsCfg<SS, D>;
  if (i >= C::TH * C::NCH) return;
  const int r = i / C::NCH, x = w.X0 + 4 * (i - r * C::NCH), y = w.Y0 + r;
  if (y > w.y1 || x > w.x1) return;
  const int nx = w.x1 + 1 - x < 4 ? w.x1 + 1 - x : 4;
  uint32_t pk[3];
  __builtin_memcpy(pk, __builtin_assume_aligned(&sh.st[(r * C::TW + (x - w.X0)) * 3], 4), 12);
  uint8_t* o = rgb + ((size_t)y * g.OW + x) * 3;
  if (nx == 4 && (((uintptr_t)o) & 3u) == 0) {
    __builtin_memcpy(__builtin_assume_aligned(o, 4), pk, 12);
  } else {
    for (int b = 0; b < 12; ++b)
      if (b < 3 * nx) o[b] = (uint8_t)(pk[b >> 2] >> (8 * (b & 3)));
  }
}

// One tile on the host: the kernel's steps with loops in place of lanes and of
// the barriers between them.  sh.q holds the image's tables.  No GPU.
template <int SS, int D>
inline void ls_host_tile(LsShared<SS, D>& sh, const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, int ty, int tx) {
  using C = LsCfg<SS, D>;
  const LsGeo g = ls_geo<SS, D>(a);
  const JWin w = ls_tile_window<SS, D>(g, ty, tx);
  if (C::WIN)
    for (int t0 = 0; t0 < 2 * w.ncbr * w.ncbc; t0 += JI_NB) {
      for (int t = t0; t < t0 + JI_NB; ++t)
        for (int v = 0; v < 8; ++v) ls_chroma_col<SS, D>(sh, a, w, coeffs, t, v);
      for (int t = t0; t < t0 + JI_NB; ++t)
        for (int u = 0; u < 8; ++u) ls_chroma_row<SS, D>(sh, a, g, w, t, u);
    }
  for (int lb = 0; lb < JI_NB; ++lb) {
    int by, bx;
    if (!ls_luma_block(a, ty, tx, lb, &by, &bx)) continue;
    int32_t* mid = sh.mid + lb * LJ_MS;
    const long long boff = ((long long)by * a.gc[0] + bx) * 64;
    int Yv[C::M][C::M], Cb[C::M][C::M] = {}, Cr[C::M][C::M] = {};
    for (int v = 0; v < 8; ++v) ls_col<C::M>(coeffs + a.off[0] + boff, sh.q, v, mid);
    for (int u = 0; u < C::M; ++u) ls_row<C::M>(mid, u, Yv[u]);
    if (SS == JDS_SS_444) {
      for (int v = 0; v < 8; ++v) ls_col<C::M>(coeffs + a.off[1] + boff, sh.q + 64, v, mid);
      for (int u = 0; u < C::M; ++u) ls_row<C::M>(mid, u, Cb[u]);
      for (int v = 0; v < 8; ++v) ls_col<C::M>(coeffs + a.off[2] + boff, sh.q + 128, v, mid);
      for (int u = 0; u < C::M; ++u) ls_row<C::M>(mid, u, Cr[u]);
    }
    for (int u = 0; u < C::M; ++u) {
      const int y = by * C::M + u, x0 = bx * C::M;
      if (y > w.y1) continue;
      if (C::WIN) {
        ls_chroma_px<SS, D>(sh, g, w, y, x0, 0, Cb[u]);
        ls_chroma_px<SS, D>(sh, g, w, y, x0, 1, Cr[u]);
      }
      ls_emit<SS, D>(sh, w, y, x0, Yv[u], Cb[u], Cr[u]);
    }
  }
  for (int i = 0; i < C::TH * C::NCH; ++i) ls_store<SS, D>(sh, g, w, rgb, i);
}

template <int SS, int D>
inline void ls_host_tables(LsShared<SS, D>& sh, const JInvArgs& a) {
  for (int c = 0; c < (SS == JDS_SS_GRAY ? 1 : 3); ++c)
    for (int i = 0; i < 64; ++i) sh.q[64 * c + i] = a.q[c][i];
}

// The host tile loop of one image.
template <int SS, int D>
inline void ls_host_image(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb) {
  LsShared<SS, D>* shp = new LsShared<SS, D>();  // (zeroed: lanes past the plane's right edge read defined samples)
  ls_host_tables<SS, D>(*shp, a);
  for (int ty = 0; ty < a.tiles_y; ++ty)
    for (int tx = 0; tx < a.tiles_x; ++tx) ls_host_tile<SS, D>(*shp, a, coeffs, rgb, ty, tx);
  delete shp;
}

// f.template operator()<SS, D>() for the mode and denominator (2, 4 or 8) named at run time.
#define LS_DISPATCH(ss, d, CALL)                                       \
  do {                                                                 \
    if ((ss) == JDS_SS_GRAY) LS_DISPATCH_D(JDS_SS_GRAY, d, CALL);      \
    else if ((ss) == JDS_SS_420) LS_DISPATCH_D(JDS_SS_420, d, CALL);   \
    else if ((ss) == JDS_SS_422) LS_DISPATCH_D(JDS_SS_422, d, CALL);   \
    else LS_DISPATCH_D(JDS_SS_444, d, CALL);                           \
  } while (0)
#define LS_DISPATCH_D(SS, d, CALL) \
  do {                             \
    if ((d) == 2) {                \
      CALL(SS, 2);                 \
    } else if ((d) == 4) {         \
      CALL(SS, 4);                 \
    } else {                       \
      CALL(SS, 8);                 \
    }                              \
  } while (0)

inline void jpeg_ljs_host_image(const JInvArgs& a, int denom, const int16_t* coeffs, uint8_t* rgb) {
#define LS_CALL_(SS, D) ls_host_image<SS, D>(a, coeffs, rgb)
  LS_DISPATCH(a.ss, denom, LS_CALL_);
#undef LS_CALL_
}

// ------------------------------------------------------------- batches --
// A record's denominator rides in JInvRec::pad_ (0 or 1: full scale, which
// stays on k_jpeg_ljt's launches and maps); its pixels are placed by its output
// size.  The scaled images get a map per (mode, denominator).

JDS_HDI int ls_rec_denom(const JInvRec& r) { return r.pad_ > 1 ? r.pad_ : 1; }

inline void ls_scaled_size(long long H, long long W, int denom, long long* oh, long long* ow) {
  *oh = (H + denom - 1) / denom;
  *ow = (W + denom - 1) / denom;
}

// jinv_batch_place with the image's output size.
inline void ls_batch_place(JInvRec& r, int k, int denom, long long coeffs_needed, long long* rgb_bytes,
                           long long* coef_entries) {
  r.coef_off = *coef_entries;
  r.rgb_off = *rgb_bytes;
  r.st = k;
  r.pad_ = denom > 1 ? denom : 0;
  *coef_entries += coeffs_needed;
  long long oh, ow;
  ls_scaled_size(r.a.H, r.a.W, denom, &oh, &ow);
  *rgb_bytes += (oh * ow * 3 + JI_RGB_ALIGN - 1) / JI_RGB_ALIGN * JI_RGB_ALIGN;
}

// jinv_batch_maps over the full-scale records alone, and a map per (mode,
// denominator index) over the scaled ones.
inline bool ls_batch_maps(const JInvRec* recs, int nrec, std::vector<JInvMap> (&map)[JI_MODES],
                          std::vector<JInvMap> (&smap)[JI_MODES][LS_ND]) {
  long long tiles[JI_MODES] = {0, 0, 0, 0}, stiles[JI_MODES][LS_ND] = {};
  for (int m = 0; m < JI_MODES; ++m) {
    map[m].clear();
    for (int d = 0; d < LS_ND; ++d) smap[m][d].clear();
  }
  for (int i = 0; i < nrec; ++i) {
    const int m = recs[i].a.ss, dn = ls_rec_denom(recs[i]);
    const long long n = (long long)recs[i].a.tiles_y * recs[i].a.tiles_x;
    std::vector<JInvMap>& mp = dn == 1 ? map[m] : smap[m][ls_denom_index(dn)];
    long long& tl = dn == 1 ? tiles[m] : stiles[m][ls_denom_index(dn)];
    mp.push_back(JInvMap{(int)tl, i});
    tl += n;
    if (tl > 0x7fffffffll) return false;
  }
  for (int m = 0; m < JI_MODES; ++m) {
    map[m].push_back(JInvMap{(int)tiles[m], -1});
    for (int d = 0; d < LS_ND; ++d) smap[m][d].push_back(JInvMap{(int)stiles[m][d], -1});
  }
  return true;
}

// The pixels of tile (ty, tx) of a flagged image: zeros.
JDS_HDI void ls_zero_lane(const LsGeo& g, const JWin& w, uint8_t* o, int i) {
  const int rb = 3 * (w.x1 - w.X0 + 1), nb = rb * (w.y1 - w.Y0 + 1);
  if (i >= nb) return;
  const int y = i / rb;
  o[((size_t)(w.Y0 + y) * g.OW + w.X0) * 3 + (i - y * rb)] = 0;
}

// The host model of one batch launch (lj_host_batch_mode's walk with this core).
template <int SS, int D>
inline void ls_host_batch_mode(const JInvRec* recs, const JInvMap* map, int nmap, const uint32_t* status,
                               const int16_t* coeffs, uint8_t* rgb) {
  using C = LsCfg<SS, D>;
  if (nmap < 1) return;
  LsShared<SS, D>* shp = new LsShared<SS, D>();
  for (int t = 0; t < map[nmap].tile0; ++t) {
    const int mi = jinv_find(map, nmap, t);
    const JInvRec& r = recs[map[mi].rec];
    const JInvArgs& a = r.a;
    const int lt = t - map[mi].tile0, ty = lt / a.tiles_x, tx = lt - ty * a.tiles_x;
    uint8_t* o = rgb + r.rgb_off;
    if (status[r.st]) {
      const LsGeo g = ls_geo<SS, D>(a);
      const JWin w = ls_tile_window<SS, D>(g, ty, tx);
      for (int i = 0; i < 3 * C::TH * C::TW; ++i) ls_zero_lane(g, w, o, i);
      continue;
    }
    ls_host_tables<SS, D>(*shp, a);
    ls_host_tile<SS, D>(*shp, a, coeffs + r.coef_off, o, ty, tx);
  }
  delete shp;
}

// smap[m][d] / nsmap[m][d]: the launch of mode m at denominator 2 << d.
inline void jpeg_ljs_batch_host(const JInvRec* recs, const JInvMap* const smap[JI_MODES][LS_ND],
                                const int nsmap[JI_MODES][LS_ND], const uint32_t* status, const int16_t* coeffs,
                                uint8_t* rgb) {
  for (int m = 0; m < JI_MODES; ++m)
    for (int d = 0; d < LS_ND; ++d) {
#define LS_CALL_(SS, D) ls_host_batch_mode<SS, D>(recs, smap[m][d], nsmap[m][d], status, coeffs, rgb)
      LS_DISPATCH(m, 2 << d, LS_CALL_);
#undef LS_CALL_
    }
}

}  // namespace jds
