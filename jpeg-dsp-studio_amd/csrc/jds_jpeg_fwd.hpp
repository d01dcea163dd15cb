// jds_jpeg_fwd.hpp — the tile core of the libjpeg encoding (jds_jpeg_fwd.hip,
// k_jpeg_fwd; DESIGN.md "libjpeg encoding"): RGB (or gray) bytes -> the
// quantised coefficients libjpeg's default compressor gives, in
// jds_decode_jpeg's planar layout: jccolor's 16-bit fixed-point conversion,
// jcsample's h2v1 / h2v2 box downsampling, jfdctint's ISLOW forward DCT and the
// rounded division by 8 q (tests/libjpeg_fwd_ref.py is the definition).  Every
// value is a 32-bit integer and none comes near its range (DESIGN.md has the
// bounds).  Compiles for host and device like jds_jpeg_ljt.hpp, whose
// arguments, tile, records and maps it shares (JInvArgs, JI_TH x JI_TW, JInvRec,
// JInvMap): the GPU lanes, the host tile loop behind jds_selftest_jpeg_forward
// and tools/jpeg_fwd_san.cpp run this same code.
//
// A tile is staged first: every lane converts patches of 4 pixels (4:2:0: 2 x 4)
// read with clamped coordinates and writes level-shifted Y samples and the
// downsampled chroma samples under them into the tile's sample planes -- the
// box filter needs no halo.  Then eight lanes own a block: lane v transforms
// row v in place, then column v, quantises it in place, and stores row v of the
// result as 16 bytes.
#pragma once
#include <stdint.h>
#include <string.h>

#include "jds.h"
#include "jds_jpeg_inv.hpp"

namespace jds {

// Row pitch of the sample planes in int16: a multiple of 8 (16-byte rows of a
// block) that is 8 mod 16 dwords, so the 16-byte row accesses of 16 lanes (two
// blocks) cover the 64 banks once.
constexpr int JF_YP = JI_TW + 16;      // luma, and 4:4:4 chroma: 72 dwords
constexpr int JF_CP = JI_TW / 2 + 16;  // chroma under horizontal subsampling: 40 dwords
static_assert(JF_YP % 8 == 0 && (JF_YP / 2) % 16 == 8 && JF_CP % 8 == 0 && (JF_CP / 2) % 16 == 8, "pitch");

// |c| entering the quantiser: the true DCT of samples in [-128, 127] is within
// 1024 (the DC of a flat block), jfdctint returns 8x that plus its rounding
// (below 8200).  The quantiser's reciprocal is proved up to here.
constexpr int JF_CBOUND = 16384;
constexpr int JF_RBITS = 20;

template <int SS>
struct JfCfg {
  static constexpr int SY = SS == JDS_SS_420 ? 2 : 1, SX = (SS == JDS_SS_422 || SS == JDS_SS_420) ? 2 : 1;
  static constexpr int NPLANES = SS == JDS_SS_GRAY ? 1 : 3;
  static constexpr int CP = SX == 2 ? JF_CP : JF_YP;       // chroma pitch
  static constexpr int CBR = JI_TH / (8 * SY), CBC = JI_TW / (8 * SX);  // chroma blocks of a tile, per plane
  static constexpr int CN = SS == JDS_SS_GRAY ? 8 : 8 * CBR * CP;
  static constexpr int NTASK = JI_NB + (SS == JDS_SS_GRAY ? 0 : 2 * CBR * CBC);
  static constexpr int NPATCH = (JI_TH / SY) * (JI_TW / 4);  // 4:2:0: 2 x 4 pixels each, else 1 x 4
};

// What one workgroup keeps in LDS (the host loop: on the heap).
template <int SS>
struct JfShared {
  alignas(16) int16_t y[JI_TH * JF_YP];
  alignas(16) int16_t c[2][JfCfg<SS>::CN];
  int q[3 * 64];
  uint32_t r[3 * 64];  // ceil(2^JF_RBITS / q)
};

JDS_HDI int jf_mul24(int a, int b) {  // both operands within 24 signed bits
#ifdef __HIP_DEVICE_COMPILE__
  return __mul24(a, b);
#else
  return a * b;
#endif
}

JDS_HDI uint32_t jf_recip(int q) { return ((1u << JF_RBITS) + (uint32_t)q - 1u) / (uint32_t)q; }

// sign(c) * ((|c| + 4 q) / (8 q)), truncating, for |c| <= JF_CBOUND and q in
// [1, 255], without a division: (|c| + 4 q) / (8 q) = m / q with
// m = (|c| + 4 q) >> 3 <= 2175, and with r = ceil(2^20 / q) = (2^20 + e) / q,
// 0 <= e < q, m r / 2^20 = m / q + m e / (q 2^20): the floor is that of m / q
// while m e < 2^20, and m e < 2176 * 255 < 2^20.  m r < 2^32 and both factors
// are within 24 bits.  tests/test_jpeg_forward_cpu.py checks every case.
JDS_HDI int jf_quant(int c, int q, uint32_t r) {
  const uint32_t a = (uint32_t)(c < 0 ? -c : c), m = (a + 4u * (uint32_t)q) >> 3;
#ifdef __HIP_DEVICE_COMPILE__
  const int t = (int)(__umul24(m, r) >> JF_RBITS);
#else
  const int t = (int)((m * r) >> JF_RBITS);
#endif
  return c < 0 ? -t : t;
}

JDS_HDI int jf_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint's 1-D pass (CONST_BITS = 13, PASS1_BITS = 2) on d[0..7] in place.
// FIRST: the row pass, results scaled up by PASS1_BITS (|.| <= 4097 for samples
// in [-128, 127]); else the column pass, which removes the scaling.
template <bool FIRST>
JDS_HDI void jf_fdct8(int (&d)[8]) {
  constexpr int N = FIRST ? 11 : 15;
  int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : jf_descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) * 4 : jf_descale(t10 - t11, 2);
  int z1 = jf_mul24(t12 + t13, 4433);
  d[2] = jf_descale(z1 + jf_mul24(t13, 6270), N);
  d[6] = jf_descale(z1 + jf_mul24(t12, -15137), N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = jf_mul24(z3 + z4, 9633);
  t4 = jf_mul24(t4, 2446);
  t5 = jf_mul24(t5, 16819);
  t6 = jf_mul24(t6, 25172);
  t7 = jf_mul24(t7, 12299);
  z1 = jf_mul24(z1, -7373);
  z2 = jf_mul24(z2, -20995);
  z3 = jf_mul24(z3, -16069) + z5;
  z4 = jf_mul24(z4, -3196) + z5;
  d[7] = jf_descale(t4 + z1 + z3, N);
  d[5] = jf_descale(t5 + z2 + z4, N);
  d[3] = jf_descale(t6 + z2 + z3, N);
  d[1] = jf_descale(t7 + z1 + z4, N);
}

// 8 int16 of a 16-byte aligned row.
JDS_HDI void jf_load8(const int16_t* p, int (&d)[8]) {
  int16_t s[8];
  __builtin_memcpy(s, (const int16_t*)__builtin_assume_aligned(p, 16), 16);
  for (int k = 0; k < 8; ++k) d[k] = s[k];
}
JDS_HDI void jf_store8(int16_t* p, const int (&d)[8]) {
  int16_t s[8];
  for (int k = 0; k < 8; ++k) s[k] = (int16_t)d[k];
  __builtin_memcpy((int16_t*)__builtin_assume_aligned(p, 16), s, 16);
}

// ------------------------------------------------------------- staging --

// n <= 16 bytes from p, all inside the image.  On the device: the aligned
// words that hold them (each holds at least one of them, so at least one byte
// of the image), shifted into place; on the host: the bytes themselves.
template <int NW>
JDS_HDI void jf_load_bytes(const uint8_t* p, uint32_t (&w)[NW]) {
#ifdef __HIP_DEVICE_COMPILE__
  const uintptr_t ad = (uintptr_t)p;
  const uint32_t sh = (uint32_t)(ad & 3u);
  const uint32_t* a = (const uint32_t*)(ad - sh);
  uint32_t v[NW + 1];
  for (int i = 0; i < NW; ++i) v[i] = a[i];
  v[NW] = sh ? a[NW] : 0u;
  for (int i = 0; i < NW; ++i) w[i] = __builtin_amdgcn_alignbyte(v[i + 1], v[i], sh);
#else
  for (int i = 0; i < NW; ++i)
    w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
#endif
}

// jccolor (SCALEBITS = 16) on one pixel; the results are in [0, 255].
JDS_HDI void jf_ycc(int R, int G, int B, int* Y, int* Cb, int* Cr) {
  *Y = (jf_mul24(19595, R) + jf_mul24(38470, G) + jf_mul24(7471, B) + 32768) >> 16;
  *Cb = (jf_mul24(-11059, R) + jf_mul24(-21709, G) + (B << 15) + (128 << 16) + 32767) >> 16;
  *Cr = ((R << 15) + jf_mul24(-27439, G) + jf_mul24(-5329, B) + (128 << 16) + 32767) >> 16;
}

// The four pixels (y, min(x + k, W - 1)), k = 0..3, of an image row y < H,
// x < W + 3 a multiple of 4: converted samples.  GRAY: Y is the byte.
template <bool GRAY>
JDS_HDI void jf_unit(const JInvArgs& a, const uint8_t* img, int y, int x, int (&Y)[4], int (&Cb)[4], int (&Cr)[4]) {
  constexpr int NC = GRAY ? 1 : 3;
  const uint8_t* row = img + (size_t)y * (size_t)a.W * NC;
  if (x + 3 < a.W) {
    uint32_t w[NC];
    jf_load_bytes<NC>(row + (size_t)x * NC, w);
    for (int k = 0; k < 4; ++k) {
      if constexpr (GRAY) {
        Y[k] = (int)((w[0] >> (8 * k)) & 255u);
      } else {
        const int b = 3 * k;
        jf_ycc((int)((w[b >> 2] >> (8 * (b & 3))) & 255u), (int)((w[(b + 1) >> 2] >> (8 * ((b + 1) & 3))) & 255u),
               (int)((w[(b + 2) >> 2] >> (8 * ((b + 2) & 3))) & 255u), &Y[k], &Cb[k], &Cr[k]);
      }
    }
    return;
  }
  for (int k = 0; k < 4; ++k) {  // the image's right edge: byte loads at clamped columns
    const uint8_t* p = row + (size_t)(x + k < a.W ? x + k : a.W - 1) * NC;
    if constexpr (GRAY)
      Y[k] = p[0];
    else
      jf_ycc(p[0], p[1], p[2], &Y[k], &Cb[k], &Cr[k]);
  }
}

JDS_HDI void jf_put4(int16_t* p, int a, int b, int c, int d) {  // (8-byte aligned)
  const int16_t s[4] = {(int16_t)a, (int16_t)b, (int16_t)c, (int16_t)d};
  __builtin_memcpy((int16_t*)__builtin_assume_aligned(p, 8), s, 8);
}
JDS_HDI void jf_put2(int16_t* p, int a, int b) {  // (4-byte aligned)
  const int16_t s[2] = {(int16_t)a, (int16_t)b};
  __builtin_memcpy((int16_t*)__builtin_assume_aligned(p, 4), s, 4);
}

// The tile's pixels (JWin's first four fields; the window fields are not used).
JDS_HDI JWin jf_tile_window(const JInvArgs& a, int ty, int tx) {
  JWin w;
  w.Y0 = ty * JI_TH;
  w.X0 = tx * JI_TW;
  w.y1 = (w.Y0 + JI_TH < a.H ? w.Y0 + JI_TH : a.H) - 1;
  w.x1 = (w.X0 + JI_TW < a.W ? w.X0 + JI_TW : a.W) - 1;
  w.wy0 = w.eh = w.wx0 = w.ew = w.cby0 = w.ncbr = w.cbx0 = w.ncbc = 0;
  return w;
}

// Patch p of the tile: 4 pixel columns of one pixel row (4:2:0: of two, one
// chroma row).  Patches beyond the samples the grids' blocks hold are skipped;
// a sample beyond the image is the image's edge pixel, except that the rows of
// a 4:2:0 chroma plane below its last one (ph - 1) repeat THAT row: libjpeg
// pads the image to an even number of rows only, downsamples, then replicates.
template <int SS>
JDS_HDI void jf_stage(JfShared<SS>& sh, const JInvArgs& a, const JWin& w, const uint8_t* img, int p) {
  using C = JfCfg<SS>;
  constexpr bool GRAY = SS == JDS_SS_GRAY;
  const int pc = p & (JI_TW / 4 - 1), pr = p / (JI_TW / 4);
  const int x = w.X0 + 4 * pc;
  const int xlim = C::SX == 2 ? 16 * a.gc[1] : 8 * a.gc[0];  // (16 gc[1] >= 8 gc[0])
  if (x >= xlim) return;
  int Y[4], Cb[4], Cr[4];
  if constexpr (C::SY == 2) {
    const int r = w.Y0 / 2 + pr;  // the chroma row
    if (r >= 8 * a.gr[1]) return;
    int Y1[4], Cb1[4], Cr1[4];
    const int y0 = 2 * r < a.H ? 2 * r : a.H - 1, y1 = 2 * r + 1 < a.H ? 2 * r + 1 : a.H - 1;
    jf_unit<false>(a, img, y0, x, Y, Cb, Cr);
    jf_unit<false>(a, img, y1, x, Y1, Cb1, Cr1);
    jf_put4(&sh.y[(2 * pr) * JF_YP + 4 * pc], Y[0] - 128, Y[1] - 128, Y[2] - 128, Y[3] - 128);
    jf_put4(&sh.y[(2 * pr + 1) * JF_YP + 4 * pc], Y1[0] - 128, Y1[1] - 128, Y1[2] - 128, Y1[3] - 128);
    if (r >= a.ph) {  // (the plane's last row lies in this tile: a tile holds whole chroma blocks)
      const int c0 = 2 * (a.ph - 1), c1 = c0 + 1 < a.H ? c0 + 1 : a.H - 1;
      jf_unit<false>(a, img, c0, x, Y, Cb, Cr);
      jf_unit<false>(a, img, c1, x, Y1, Cb1, Cr1);
    }
    jf_put2(&sh.c[0][pr * C::CP + 2 * pc], ((Cb[0] + Cb[1] + Cb1[0] + Cb1[1] + 1) >> 2) - 128,
            ((Cb[2] + Cb[3] + Cb1[2] + Cb1[3] + 2) >> 2) - 128);
    jf_put2(&sh.c[1][pr * C::CP + 2 * pc], ((Cr[0] + Cr[1] + Cr1[0] + Cr1[1] + 1) >> 2) - 128,
            ((Cr[2] + Cr[3] + Cr1[2] + Cr1[3] + 2) >> 2) - 128);
  } else {
    const int yy = w.Y0 + pr;
    if (yy >= 8 * a.gr[0]) return;
    jf_unit<GRAY>(a, img, yy < a.H ? yy : a.H - 1, x, Y, Cb, Cr);
    jf_put4(&sh.y[pr * JF_YP + 4 * pc], Y[0] - 128, Y[1] - 128, Y[2] - 128, Y[3] - 128);
    if constexpr (C::SX == 2) {
      jf_put2(&sh.c[0][pr * C::CP + 2 * pc], ((Cb[0] + Cb[1]) >> 1) - 128, ((Cb[2] + Cb[3] + 1) >> 1) - 128);
      jf_put2(&sh.c[1][pr * C::CP + 2 * pc], ((Cr[0] + Cr[1]) >> 1) - 128, ((Cr[2] + Cr[3] + 1) >> 1) - 128);
    } else if constexpr (!GRAY) {
      jf_put4(&sh.c[0][pr * C::CP + 4 * pc], Cb[0] - 128, Cb[1] - 128, Cb[2] - 128, Cb[3] - 128);
      jf_put4(&sh.c[1][pr * C::CP + 4 * pc], Cr[0] - 128, Cr[1] - 128, Cr[2] - 128, Cr[3] - 128);
    }
  }
}

// -------------------------------------------------------------- blocks --

// Block task t of a tile: its JI_NB luma blocks in raster order, then the Cb
// and the Cr blocks under them.  blk: the block's samples in the tile's planes.
struct JfTask {
  int c, pitch;
  long long out;  // the block's first coefficient
  int16_t* blk;
  bool ok;        // inside the component's grid
};
template <int SS>
JDS_HDI JfTask jf_task(JfShared<SS>& sh, const JInvArgs& a, const JWin& w, int t) {
  using C = JfCfg<SS>;
  JfTask k;
  int by, bx;
  if (SS == JDS_SS_GRAY || t < JI_NB) {
    const int bi = t / (JI_TW / 8), bj = t - bi * (JI_TW / 8);
    k.c = 0;
    k.pitch = JF_YP;
    k.blk = &sh.y[bi * 8 * JF_YP + bj * 8];
    by = w.Y0 / 8 + bi;
    bx = w.X0 / 8 + bj;
  } else {
    const int u = t - JI_NB, p = u / (C::CBR * C::CBC), b = u - p * (C::CBR * C::CBC);
    const int bi = b / C::CBC, bj = b - bi * C::CBC;
    k.c = 1 + p;
    k.pitch = C::CP;
    k.blk = &sh.c[p][bi * 8 * C::CP + bj * 8];
    by = w.Y0 / (8 * C::SY) + bi;
    bx = w.X0 / (8 * C::SX) + bj;
  }
  const int gr = k.c ? a.gr[1] : a.gr[0], gc = k.c ? a.gc[1] : a.gc[0];
  k.ok = t < C::NTASK && by < gr && bx < gc;
  k.out = (k.c == 0 ? a.off[0] : (k.c == 1 ? a.off[1] : a.off[2])) + ((long long)by * gc + bx) * 64;
  return k;
}

// Lane v of a block's eight: row v in place (the row pass; its results fit int16).
JDS_HDI void jf_rows(const JfTask& k, int v) {
  int d[8];
  jf_load8(k.blk + v * k.pitch, d);
  jf_fdct8<true>(d);
  jf_store8(k.blk + v * k.pitch, d);
}

// Column v: the column pass and the quantiser, in place.
JDS_HDI void jf_cols(const JfTask& k, const int* q, const uint32_t* r, int v) {
  int d[8];
  for (int i = 0; i < 8; ++i) d[i] = k.blk[i * k.pitch + v];
  jf_fdct8<false>(d);
  for (int i = 0; i < 8; ++i) k.blk[i * k.pitch + v] = (int16_t)jf_quant(d[i], q[64 * k.c + 8 * i + v], r[64 * k.c + 8 * i + v]);
}

// Row v of the quantised block: 16 bytes out (coeffs + k.out is 16-byte aligned).
JDS_HDI void jf_out(const JfTask& k, int16_t* coeffs, int v) {
  int16_t* o = coeffs + k.out + 8 * v;
  __builtin_memcpy((int16_t*)__builtin_assume_aligned(o, 16), (const int16_t*)__builtin_assume_aligned(k.blk + v * k.pitch, 16), 16);
}

// ------------------------------------------------------- host tile loop --

// The tables of an image into sh.q / sh.r (grayscale: component 0 alone).
template <int SS>
inline void jf_host_tables(JfShared<SS>& sh, const JInvArgs& a) {
  for (int c = 0; c < JfCfg<SS>::NPLANES; ++c)
    for (int i = 0; i < 64; ++i) {
      sh.q[64 * c + i] = a.q[c][i];
      sh.r[64 * c + i] = jf_recip(a.q[c][i]);
    }
}

// One tile on the host: the kernel's steps with loops in place of lanes and of
// the barriers between them.  No GPU.
template <int SS>
inline void jf_host_tile(JfShared<SS>& sh, const JInvArgs& a, const uint8_t* img, int16_t* coeffs, int ty, int tx) {
  using C = JfCfg<SS>;
  const JWin w = jf_tile_window(a, ty, tx);
  for (int p = 0; p < C::NPATCH; ++p) jf_stage<SS>(sh, a, w, img, p);
  for (int t = 0; t < C::NTASK; ++t) {
    const JfTask k = jf_task<SS>(sh, a, w, t);
    if (!k.ok) continue;
    for (int v = 0; v < 8; ++v) jf_rows(k, v);
    for (int v = 0; v < 8; ++v) jf_cols(k, sh.q, sh.r, v);
    for (int v = 0; v < 8; ++v) jf_out(k, coeffs, v);
  }
}

template <int SS>
inline void jf_host_image(const JInvArgs& a, const uint8_t* img, int16_t* coeffs) {
  JfShared<SS>* shp = new JfShared<SS>();
  jf_host_tables<SS>(*shp, a);
  for (int ty = 0; ty < a.tiles_y; ++ty)
    for (int tx = 0; tx < a.tiles_x; ++tx) jf_host_tile<SS>(*shp, a, img, coeffs, ty, tx);
  delete shp;
}

// The host tile loop of one image; coeffs: 16-byte aligned.
inline void jpeg_fwd_host_image(const JInvArgs& a, const uint8_t* img, int16_t* coeffs) {
  if (a.ss == JDS_SS_GRAY)
    jf_host_image<JDS_SS_GRAY>(a, img, coeffs);
  else if (a.ss == JDS_SS_420)
    jf_host_image<JDS_SS_420>(a, img, coeffs);
  else if (a.ss == JDS_SS_422)
    jf_host_image<JDS_SS_422>(a, img, coeffs);
  else
    jf_host_image<JDS_SS_444>(a, img, coeffs);
}

// ------------------------------------------------------------- tables --

// T.81 Annex K.1 / K.2, row-major.
constexpr uint8_t JF_BASE[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// jpeg_set_quality(quality, force_baseline) for quality in [1, 100]: table t (0 luma, 1 chroma).
inline void jf_quality_table(int quality, int t, double* out) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    const int v = (JF_BASE[t][i] * s + 50) / 100;
    out[i] = (double)(v < 1 ? 1 : (v > 255 ? 255 : v));
  }
}

// The info of an H x W image encoded at a quality: geometry (T.81's grids),
// tq = (0, 1, 1) and the tables; a grayscale one: one component, table 0.
// Scans and Huffman tables stay zero.  The arguments are the caller's to check.
inline void jf_quality_info(int quality, int ss, int64_t H, int64_t W, jds_jpeg_info* out) {
  memset(out, 0, sizeof *out);
  out->H = H;
  out->W = W;
  out->subsampling = ss;
  out->n_scans = 1;
  const int ncomp = ss == JDS_SS_GRAY ? 1 : 3;
  const int hmax = (ss == JDS_SS_422 || ss == JDS_SS_420) ? 2 : 1, vmax = ss == JDS_SS_420 ? 2 : 1;
  out->interleaved = ncomp == 3;
  out->single_table = ncomp == 1;
  out->blocks_per_mcu = ncomp == 1 ? 1 : hmax * vmax + 2;
  for (int c = 0; c < ncomp; ++c) {
    out->hs[c] = c ? 1 : hmax;
    out->vs[c] = c ? 1 : vmax;
    out->tq[c] = c ? 1 : 0;
    const int64_t xc = c ? (W + hmax - 1) / hmax : W, yc = c ? (H + vmax - 1) / vmax : H;
    out->grid_cols[c] = (xc + 7) / 8;
    out->grid_rows[c] = (yc + 7) / 8;
    out->coeffs_needed += 64 * out->grid_cols[c] * out->grid_rows[c];
    jf_quality_table(quality, c ? 1 : 0, out->qtable[c]);
  }
  out->mcu_cols = (W + 8 * hmax - 1) / (8 * hmax);
  out->mcu_rows = (H + 8 * vmax - 1) / (8 * vmax);
  if (ncomp == 1) {
    out->hs[0] = out->vs[0] = 1;
    out->mcu_cols = out->grid_cols[0];
    out->mcu_rows = out->grid_rows[0];
  }
}

}  // namespace jds
