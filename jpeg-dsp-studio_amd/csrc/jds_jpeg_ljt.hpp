// jds_jpeg_ljt.hpp — the tile core of the libjpeg rendering (jds_jpeg_ljt.hip,
// k_jpeg_ljt; DESIGN.md "libjpeg rendering"): decoded coefficients in
// jds_decode_jpeg's layout -> the RGB bytes libjpeg's default decode gives:
// jidctint's ISLOW inverse, jdsample's fancy upsampling, jdcolor's 16-bit
// fixed-point conversion (tests/libjpeg_ref.py is the definition).  Every value
// is a 32-bit integer; sums and products are taken modulo 2^32 on the unsigned
// view and shifted arithmetically on the signed one, so no coefficient can
// reach undefined behaviour and kernel, host loop and reference agree on every
// int16 input.  Compiles for host and device like jds_jpeg_inv.hpp, whose
// arguments, tile, records and maps it shares (JInvArgs, JI_TH x JI_TW, JInvRec,
// JInvMap): the GPU lanes, the host tile loop behind jds_selftest_jpeg_render
// and tools/jpeg_ljt_san.cpp run this same code.
//
// Eight lanes own a block: lane v transforms column v into the transpose
// buffer, then row v out of it.  With subsampled chroma a tile first transforms
// the chroma blocks under it into a window of samples -- the tile's own chroma
// samples and one sample of halo on each subsampled axis, a sample outside the
// file's T.81 plane being the plane's edge sample -- then its luma blocks, whose
// row pass upsamples with libjpeg's fixed taps, converts and stores 8 pixels.
#pragma once
#include <stdint.h>
#include <string.h>

#include "jds.h"
#include "jds_jpeg_inv.hpp"

namespace jds {

constexpr int LJ_MS = 72;  // int32 per block in the transpose buffer: 64 + 8, so the 8 blocks of a wave start 8 banks apart
constexpr int LJ_WS = 96;  // int16 per window row: 48 dwords, so consecutive rows start 16 banks apart (mod 64)

template <int SS>
struct LjCfg {
  static constexpr int SY = SS == JDS_SS_420 ? 2 : 1, SX = (SS == JDS_SS_422 || SS == JDS_SS_420) ? 2 : 1;
  static constexpr int CWR = SY == 2 ? JI_TH / 2 + 2 : JI_TH;  // window rows
  static constexpr int CWC = JI_TW / 2 + 2;                    // window columns
  static constexpr int CWN = SX == 2 ? CWR * LJ_WS : 4;        // 4:4:4 and gray have no window
};
static_assert(LjCfg<JDS_SS_420>::CWC <= LJ_WS && LJ_WS % 4 == 0, "window row");

// What one workgroup keeps in LDS (the host loop: on the heap).
template <int SS>
struct LjShared {
  int32_t mid[JI_NB * LJ_MS];
  alignas(8) int16_t cw[2][LjCfg<SS>::CWN];
  int q[3 * 64];
};

// Element (r, c) of a block in the transpose buffer.  Lane v writes column v: 8
// lanes fill 8 consecutive dwords of row r (permuted), the wave's 8 blocks 8
// banks apart.  Lane u reads row u: at step k the lanes of a block sit 8 dwords
// apart and the blocks 72, and c ^ r separates what 8 (u + b) brings together.
JDS_HDI int lj_slot(int r, int c) { return r * 8 + (c ^ r); }

JDS_HDI int lj_mul24(int a, int b) {  // both operands within 24 signed bits
#ifdef __HIP_DEVICE_COMPILE__
  return __mul24(a, b);
#else
  return a * b;
#endif
}

JDS_HDI int32_t lj_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }

// jidctint's 1-D pass (CONST_BITS = 13) on in[0..7], each output DESCALEd by N.
template <int N>
JDS_HDI void lj_idct8(const int32_t (&in)[8], int32_t (&out)[8]) {
  uint32_t i[8];
  for (int k = 0; k < 8; ++k) i[k] = (uint32_t)in[k];
  uint32_t z1 = (i[2] + i[6]) * 4433u;
  const uint32_t tmp2 = z1 - i[6] * 15137u, tmp3 = z1 + i[2] * 6270u;
  const uint32_t tmp0 = (i[0] + i[4]) << 13, tmp1 = (i[0] - i[4]) << 13;
  const uint32_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  uint32_t a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  a0 *= 2446u;
  a1 *= 16819u;
  a2 *= 25172u;
  a3 *= 12299u;
  z1 *= 0u - 7373u;
  z2 *= 0u - 20995u;
  z3 = z3 * (0u - 16069u) + z5;
  z4 = z4 * (0u - 3196u) + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  out[0] = lj_descale(t10 + a3, N);
  out[1] = lj_descale(t11 + a2, N);
  out[2] = lj_descale(t12 + a1, N);
  out[3] = lj_descale(t13 + a0, N);
  out[4] = lj_descale(t13 - a0, N);
  out[5] = lj_descale(t12 - a1, N);
  out[6] = lj_descale(t11 - a2, N);
  out[7] = lj_descale(t10 - a3, N);
}

// Dequantise (|coefficient| < 2^15, Q <= 255: within 24 bits) and transform
// column v of a block: the first pass, DESCALE(., CONST_BITS - PASS1_BITS).
JDS_HDI void lj_col(const int16_t* blk, const int* q, int v, int32_t* mid) {
  int32_t c[8], o[8];
  for (int r = 0; r < 8; ++r) c[r] = lj_mul24((int)blk[r * 8 + v], q[r * 8 + v]);
  lj_idct8<11>(c, o);
  for (int r = 0; r < 8; ++r) mid[lj_slot(r, v)] = o[r];
}

// Row u: the second pass, DESCALE(., CONST_BITS + PASS1_BITS + 3), + 128, clamp.
JDS_HDI void lj_row(const int32_t* mid, int u, int (&c)[8]) {
  int32_t in[8], o[8];
  for (int k = 0; k < 8; ++k) in[k] = mid[lj_slot(u, k)];
  lj_idct8<18>(in, o);
  for (int k = 0; k < 8; ++k) c[k] = jinv_clamp((int32_t)((uint32_t)o[k] + 128u), 0, 255);
}

// The tile's pixels, its window's origin (wy0 / wx0: the sample one above /
// left of the tile's first chroma sample, -1 at the image's edge) and the
// chroma blocks that hold the window's samples inside the plane.
template <int SS>
JDS_HDI JWin lj_tile_window(const JInvArgs& a, int ty, int tx) {
  using C = LjCfg<SS>;
  JWin w;
  w.Y0 = ty * JI_TH;
  w.X0 = tx * JI_TW;
  w.y1 = (w.Y0 + JI_TH < a.H ? w.Y0 + JI_TH : a.H) - 1;
  w.x1 = (w.X0 + JI_TW < a.W ? w.X0 + JI_TW : a.W) - 1;
  w.wy0 = C::SY == 2 ? w.Y0 / 2 - 1 : w.Y0;
  w.eh = C::CWR;
  w.wx0 = C::SX == 2 ? w.X0 / 2 - 1 : 0;
  w.ew = C::CWC;
  w.cby0 = w.ncbr = w.cbx0 = w.ncbc = 0;
  if (C::SX == 2) {
    const int ylo = w.wy0 < 0 ? 0 : w.wy0, yhi = w.wy0 + C::CWR - 1 < a.ph - 1 ? w.wy0 + C::CWR - 1 : a.ph - 1;
    const int xlo = w.wx0 < 0 ? 0 : w.wx0, xhi = w.wx0 + C::CWC - 1 < a.pw - 1 ? w.wx0 + C::CWC - 1 : a.pw - 1;
    w.cby0 = ylo / 8;
    w.ncbr = yhi / 8 - w.cby0 + 1;
    w.cbx0 = xlo / 8;
    w.ncbc = xhi / 8 - w.cbx0 + 1;
  }
  return w;
}

template <int SS>
JDS_HDI void lj_chroma_col(LjShared<SS>& sh, const JInvArgs& a, const JWin& w, const int16_t* coeffs, int t, int v) {
  const JTask k = jinv_chroma_task(a, w, t);
  if (!k.ok) return;
  lj_col(coeffs + a.off[1 + k.p] + ((long long)k.by * a.gc[1] + k.bx) * 64, sh.q + 64 * (1 + k.p), v,
         sh.mid + (t % JI_NB) * LJ_MS);
}

// Row u of the block goes into the window where the window holds it.  Only
// samples of the file's plane (ph x pw) are written, never the block padding;
// a sample on the plane's edge is also written one place outside it, which is
// what libjpeg's edge cases read (its first and last columns, its row context
// at the top and bottom of the image).
template <int SS>
JDS_HDI void lj_chroma_row(LjShared<SS>& sh, const JInvArgs& a, const JWin& w, int t, int u) {
  using C = LjCfg<SS>;
  const JTask k = jinv_chroma_task(a, w, t);
  const int cy = k.by * 8 + u;
  if (!k.ok || cy >= a.ph) return;
  const int wr0 = cy - w.wy0;
  if (wr0 < -1 || wr0 > C::CWR) return;
  int c[8];
  lj_row(sh.mid + (t % JI_NB) * LJ_MS, u, c);
  for (int dy = -1; dy <= 1; ++dy) {
    if (dy == -1 && !(C::SY == 2 && cy == 0)) continue;
    if (dy == 1 && !(C::SY == 2 && cy == a.ph - 1)) continue;
    const int wr = wr0 + dy;
    if (wr < 0 || wr >= C::CWR) continue;
    int16_t* row = &sh.cw[k.p][C::SX == 2 ? wr * LJ_WS : 0];
    for (int j = 0; j < 8; ++j) {
      const int cx = k.bx * 8 + j, wc = cx - w.wx0;
      if (cx >= a.pw) break;
      if (wc >= 0 && wc < C::CWC) row[wc] = (int16_t)c[j];
      if (cx == 0 && wc >= 1 && wc - 1 < C::CWC) row[wc - 1] = (int16_t)c[j];
      if (cx == a.pw - 1 && wc + 1 >= 0 && wc + 1 < C::CWC) row[wc + 1] = (int16_t)c[j];
    }
  }
}

// One plane's upsampled chroma at the 8 pixels from column x0 of row y:
// jdsample's h2v1 / h2v2 fancy taps on the six window samples around the four
// under the pixels (two window rows with vertical subsampling); plain
// replication when the plane is at most two samples wide, as libjpeg chooses.
template <int SS>
JDS_HDI void lj_chroma_up(const LjShared<SS>& sh, const JInvArgs& a, const JWin& w, int y, int x0, int p, int (&Cv)[8]) {
  using C = LjCfg<SS>;
  const int r0 = (C::SY == 2 ? (y >> 1) : y) - w.wy0, r1 = C::SY == 2 ? ((y & 1) ? r0 + 1 : r0 - 1) : r0;
  const int c0 = (x0 - w.X0) >> 1;  // a multiple of 4: the reads below are 8- and 4-byte aligned
  int16_t s0[8], s1[8];
  const int16_t* p0 = (const int16_t*)__builtin_assume_aligned(&sh.cw[p][C::SX == 2 ? r0 * LJ_WS + c0 : 0], 8);
  __builtin_memcpy(s0, p0, 8);
  __builtin_memcpy(s0 + 4, p0 + 4, 4);
  if (a.pw <= 2) {
    for (int k = 0; k < 8; ++k) Cv[k] = s0[1 + (k >> 1)];
    return;
  }
  if (C::SY == 2) {
    const int16_t* p1 = (const int16_t*)__builtin_assume_aligned(&sh.cw[p][C::SX == 2 ? r1 * LJ_WS + c0 : 0], 8);
    __builtin_memcpy(s1, p1, 8);
    __builtin_memcpy(s1 + 4, p1 + 4, 4);
    int t[6];
    for (int j = 0; j < 6; ++j) t[j] = 3 * s0[j] + s1[j];
    for (int i = 0; i < 4; ++i) {
      Cv[2 * i] = (3 * t[i + 1] + t[i] + 8) >> 4;
      Cv[2 * i + 1] = (3 * t[i + 1] + t[i + 2] + 7) >> 4;
    }
  } else {
    for (int i = 0; i < 4; ++i) {
      Cv[2 * i] = (3 * s0[i + 1] + s0[i] + 1) >> 2;
      Cv[2 * i + 1] = (3 * s0[i + 1] + s0[i + 2] + 2) >> 2;
    }
  }
}

// Four values into the bytes of one word, each clamped to [0, 255] (on the
// device the saturating pack of the fast inverse: the values fit int16).
JDS_HDI uint32_t lj_pack4(int a, int b, int c, int d) {
#ifdef __HIP_DEVICE_COMPILE__
  uint32_t ab, cd;
  asm("v_sat_pk_u8_i16 %0, %1" : "=v"(ab) : "v"(__builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x05040100u)));
  asm("v_sat_pk_u8_i16 %0, %1" : "=v"(cd) : "v"(__builtin_amdgcn_perm((uint32_t)d, (uint32_t)c, 0x05040100u)));
  return ab | (cd << 16);
#else
  return (uint32_t)jinv_clamp(a, 0, 255) | (uint32_t)jinv_clamp(b, 0, 255) << 8 | (uint32_t)jinv_clamp(c, 0, 255) << 16 |
         (uint32_t)jinv_clamp(d, 0, 255) << 24;
#endif
}

// 24 channel values (8 pixels) as packed bytes, the first nx pixels at o.
JDS_HDI void lj_store24(const int (&ch)[24], uint8_t* o, int nx) {
  uint32_t pk[6];
  for (int i = 0; i < 6; ++i) pk[i] = lj_pack4(ch[4 * i], ch[4 * i + 1], ch[4 * i + 2], ch[4 * i + 3]);
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

// jdcolor (SCALEBITS = 16): the products stay within 2^31 for samples in
// [0, 255] and both factors within 24 bits.
JDS_HDI void lj_colour_store(const int (&Yv)[8], const int (&Cb)[8], const int (&Cr)[8], uint8_t* o, int nx) {
  int ch[24];
  for (int k = 0; k < 8; ++k) {
    const int cb = Cb[k] - 128, cr = Cr[k] - 128;
    ch[3 * k] = Yv[k] + ((lj_mul24(91881, cr) + 32768) >> 16);
    ch[3 * k + 1] = Yv[k] + ((lj_mul24(-22554, cb) + lj_mul24(-46802, cr) + 32768) >> 16);
    ch[3 * k + 2] = Yv[k] + ((lj_mul24(116130, cb) + 32768) >> 16);
  }
  lj_store24(ch, o, nx);
}

JDS_HDI void lj_gray_store(const int (&Yv)[8], uint8_t* o, int nx) {
  int ch[24];
  for (int k = 0; k < 8; ++k) ch[3 * k] = ch[3 * k + 1] = ch[3 * k + 2] = Yv[k];
  lj_store24(ch, o, nx);
}

// One tile on the host: the kernel's steps with loops in place of lanes and of
// the barriers between them.  sh.q holds the image's tables.  No GPU.
template <int SS>
inline void lj_host_tile(LjShared<SS>& sh, const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, int ty, int tx) {
  using C = LjCfg<SS>;
  const JWin w = lj_tile_window<SS>(a, ty, tx);
  if (C::SX == 2)
    for (int t0 = 0; t0 < 2 * w.ncbr * w.ncbc; t0 += JI_NB) {
      for (int t = t0; t < t0 + JI_NB; ++t)
        for (int v = 0; v < 8; ++v) lj_chroma_col<SS>(sh, a, w, coeffs, t, v);
      for (int t = t0; t < t0 + JI_NB; ++t)
        for (int u = 0; u < 8; ++u) lj_chroma_row<SS>(sh, a, w, t, u);
    }
  for (int lb = 0; lb < JI_NB; ++lb) {
    int by, bx;
    if (!jinv_luma_block(a, w, lb, &by, &bx)) continue;
    int32_t* mid = sh.mid + lb * LJ_MS;
    const long long boff = ((long long)by * a.gc[0] + bx) * 64;
    int Yv[8][8], Cb[8][8], Cr[8][8];
    for (int v = 0; v < 8; ++v) lj_col(coeffs + a.off[0] + boff, sh.q, v, mid);
    for (int u = 0; u < 8; ++u) lj_row(mid, u, Yv[u]);
    if (SS == JDS_SS_444) {
      for (int v = 0; v < 8; ++v) lj_col(coeffs + a.off[1] + boff, sh.q + 64, v, mid);
      for (int u = 0; u < 8; ++u) lj_row(mid, u, Cb[u]);
      for (int v = 0; v < 8; ++v) lj_col(coeffs + a.off[2] + boff, sh.q + 128, v, mid);
      for (int u = 0; u < 8; ++u) lj_row(mid, u, Cr[u]);
    }
    for (int u = 0; u < 8; ++u) {
      const int y = by * 8 + u, x0 = bx * 8;
      if (y > w.y1) continue;
      const int nx = w.x1 + 1 - x0 < 8 ? w.x1 + 1 - x0 : 8;
      uint8_t* o = rgb + ((size_t)y * a.W + x0) * 3;
      if (SS == JDS_SS_GRAY) {
        lj_gray_store(Yv[u], o, nx);
        continue;
      }
      if (C::SX == 2) {
        lj_chroma_up<SS>(sh, a, w, y, x0, 0, Cb[u]);
        lj_chroma_up<SS>(sh, a, w, y, x0, 1, Cr[u]);
      }
      lj_colour_store(Yv[u], Cb[u], Cr[u], o, nx);
    }
  }
}

// The tables of an image into sh.q (grayscale: component 0 alone is defined).
template <int SS>
inline void lj_host_tables(LjShared<SS>& sh, const JInvArgs& a) {
  for (int c = 0; c < (SS == JDS_SS_GRAY ? 1 : 3); ++c)
    for (int i = 0; i < 64; ++i) sh.q[64 * c + i] = a.q[c][i];
}

// The host tile loop of one image.
template <int SS>
inline void lj_host_image(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb) {
  LjShared<SS>* shp = new LjShared<SS>();  // (zeroed: lanes past the plane's right edge read defined samples)
  lj_host_tables<SS>(*shp, a);
  for (int ty = 0; ty < a.tiles_y; ++ty)
    for (int tx = 0; tx < a.tiles_x; ++tx) lj_host_tile<SS>(*shp, a, coeffs, rgb, ty, tx);
  delete shp;
}

inline void jpeg_ljt_host_image(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb) {
  if (a.ss == JDS_SS_GRAY)
    lj_host_image<JDS_SS_GRAY>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_420)
    lj_host_image<JDS_SS_420>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_422)
    lj_host_image<JDS_SS_422>(a, coeffs, rgb);
  else
    lj_host_image<JDS_SS_444>(a, coeffs, rgb);
}

// The host model of the batch launches (jinv_host_batch_mode's walk with this
// tile core): a flagged image's tiles are zero-filled, nothing between images
// is written.
template <int SS>
inline void lj_host_batch_mode(const JInvRec* recs, const JInvMap* map, int nmap, const uint32_t* status,
                               const int16_t* coeffs, uint8_t* rgb) {
  if (nmap < 1) return;
  LjShared<SS>* shp = new LjShared<SS>();
  for (int t = 0; t < map[nmap].tile0; ++t) {
    const int mi = jinv_find(map, nmap, t);
    const JInvRec& r = recs[map[mi].rec];
    const JInvArgs& a = r.a;
    const int lt = t - map[mi].tile0, ty = lt / a.tiles_x, tx = lt - ty * a.tiles_x;
    uint8_t* o = rgb + r.rgb_off;
    if (status[r.st]) {
      const JWin w = lj_tile_window<SS>(a, ty, tx);
      for (int y = w.Y0; y <= w.y1; ++y) memset(o + ((size_t)y * a.W + w.X0) * 3, 0, 3 * (size_t)(w.x1 - w.X0 + 1));
      continue;
    }
    lj_host_tables<SS>(*shp, a);
    lj_host_tile<SS>(*shp, a, coeffs + r.coef_off, o, ty, tx);
  }
  delete shp;
}

inline void jpeg_ljt_batch_host(const JInvRec* recs, const JInvMap* const map[JI_MODES], const int nmap[JI_MODES],
                                const uint32_t* status, const int16_t* coeffs, uint8_t* rgb) {
  lj_host_batch_mode<JDS_SS_444>(recs, map[JDS_SS_444], nmap[JDS_SS_444], status, coeffs, rgb);
  lj_host_batch_mode<JDS_SS_422>(recs, map[JDS_SS_422], nmap[JDS_SS_422], status, coeffs, rgb);
  lj_host_batch_mode<JDS_SS_420>(recs, map[JDS_SS_420], nmap[JDS_SS_420], status, coeffs, rgb);
  lj_host_batch_mode<JDS_SS_GRAY>(recs, map[JDS_SS_GRAY], nmap[JDS_SS_GRAY], status, coeffs, rgb);
}

}  // namespace jds
