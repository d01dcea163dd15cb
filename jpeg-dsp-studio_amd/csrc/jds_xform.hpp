// jds_xform.hpp — what the lossless transforms (DESIGN.md "Lossless
// transforms"; byte-for-byte definition: tests/transform_ref.py) share between
// the kernel (jds_xform.hip), the C-ABI, the host model
// (jds_selftest_jpeg_transform) and the stand-alone sanitizer program
// (tools/jpeg_xform_san.cpp): the operations as three flags, the geometry
// rules (whole-MCU mirror axes, trim, no transposition at 4:2:2), the per-file
// record of the kernel, the destination -> source block map, the host
// coefficient transform, the EXIF Orientation reader and the prefix editor.
// Compiles for host and device.  No HIP types here.
//
// EXIF: only the Orientation tag (0x0112) of IFD0 is read and, under
// JDS_XF_AUTO, reset to 1.  Every other EXIF field stays as it is: the pixel
// dimension tags (0xA002 / 0xA003), the thumbnail of IFD1 and its own
// orientation are NOT updated.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "jds.h"
#include "jds_entropy_mcu.hpp"

namespace jds {

// An operation is: transpose the (cropped) source or not, then mirror the
// result left-right (XF_FH) and / or top-bottom (XF_FV).
constexpr int XF_T = 1, XF_FH = 2, XF_FV = 4;

// flags of an operation 0..7; -1: no such operation
JDS_MCU int xf_flags(int op) {
  switch (op) {
    case JDS_XF_NONE: return 0;
    case JDS_XF_HFLIP: return XF_FH;
    case JDS_XF_VFLIP: return XF_FV;
    case JDS_XF_TRANSPOSE: return XF_T;
    case JDS_XF_TRANSVERSE: return XF_T | XF_FH | XF_FV;  // transpose, then rot180
    case JDS_XF_ROT90: return XF_T | XF_FH;               // transpose, then hflip
    case JDS_XF_ROT180: return XF_FH | XF_FV;
    case JDS_XF_ROT270: return XF_T | XF_FV;              // hflip, then transpose = transpose, then vflip
    default: return -1;
  }
}

constexpr int XF_BLOCKS = 32;  // destination blocks of a tile (one workgroup: 8 lanes per block)

// One transformed file of a launch.  Offsets count from the coefficient base,
// as McuFile::off does.
struct XfFile {
  int32_t flags;            // XF_T | XF_FH | XF_FV
  int32_t tile0;            // its first tile in the launch's tile table
  int32_t ctile[3];         // a component's first tile, counted from tile0
  int32_t sgw[3];           // the source planes' grid columns (the stored row length)
  int32_t xr[3], xc[3];     // the cropped source grid: rows, columns (trim drops the partial MCU row / column)
  int32_t dgw[3], dgh[3];   // the destination grids: columns, rows
  int64_t soff[3], doff[3];  // the planes' first coefficients: source, destination
};

// The source block of destination block (r, c) of a component: its first
// coefficient.  X = the cropped source, transposed with XF_T; the destination
// is X mirrored.
JDS_MCU long long xf_src_block(int flags, int dgw, int dgh, int sgw, long long soff, int r, int c) {
  const int a = (flags & XF_FV) ? dgh - 1 - r : r, b = (flags & XF_FH) ? dgw - 1 - c : c;
  const int sr = (flags & XF_T) ? b : a, sc = (flags & XF_T) ? a : b;
  return soff + 64ll * ((long long)sr * sgw + sc);
}

// -x in 32 bits, the low half kept: -(-32768) is -32768, as NumPy's int16 wraps
JDS_MCU int16_t xf_neg16(int16_t x) { return (int16_t)(uint16_t)(0u - (uint32_t)(int32_t)x); }

// tiles of a record whose grids are set: fills tile0 and ctile, returns the count
inline int64_t xf_set_tiles(XfFile* f, int64_t tile0) {
  int64_t t = 0;
  for (int c = 0; c < 3; ++c) {
    f->ctile[c] = (int32_t)t;
    t += ((int64_t)f->dgw[c] * f->dgh[c] + XF_BLOCKS - 1) / XF_BLOCKS;
  }
  f->tile0 = (int32_t)tile0;
  return t;
}

// The coefficient transform on the host, block by block through the kernel's
// own block map.  src, dst: the bases the record's offsets count from.
inline void xf_host(const XfFile& f, const int16_t* src, int16_t* dst) {
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < f.dgh[c]; ++r)
      for (int q = 0; q < f.dgw[c]; ++q) {
        const int16_t* s = src + xf_src_block(f.flags, f.dgw[c], f.dgh[c], f.sgw[c], f.soff[c], r, q);
        int16_t* d = dst + f.doff[c] + 64ll * ((long long)r * f.dgw[c] + q);
        for (int v = 0; v < 8; ++v)
          for (int u = 0; u < 8; ++u) {
            const int16_t x = (f.flags & XF_T) ? s[8 * u + v] : s[8 * v + u];
            const bool neg = (((f.flags & XF_FH) && (u & 1)) != ((f.flags & XF_FV) && (v & 1)));
            d[8 * v + u] = neg ? xf_neg16(x) : x;
          }
      }
}

// --------------------------------------------------------------- plan --

struct XfPlan {
  int op;             // 0..7, JDS_XF_AUTO resolved
  int flags;
  int64_t cH, cW;     // the source after trim
  jds_jpeg_info dst;  // H, W, subsampling, grids and coeffs_needed of the output
  XfFile rec;         // offsets from 0 on both sides, tiles from 0
  int64_t tiles;
};

// The geometry of `op` (0..7) on a parsed file.  JDS_OK; JDS_ENOTSUP: a
// transposing operation at 4:2:2, or without `trim` a mirrored axis that is
// not whole MCUs; JDS_EINVAL: the trim leaves nothing, no such operation.
inline int xf_plan(const jds_jpeg_info* info, int op, bool trim, XfPlan* p, char* msg, size_t msg_n) {
  memset(p, 0, sizeof *p);
  const int flags = xf_flags(op);
  McuFile sf;
  if (flags < 0) {
    snprintf(msg, msg_n, "unknown transform operation %d", op);
    return JDS_EINVAL;
  }
  if (mcu_file_of(info, &sf)) {
    snprintf(msg, msg_n, "transform: the block grids are not the T.81 grids of %lldx%lld", (long long)info->H,
             (long long)info->W);
    return JDS_EINVAL;
  }
  p->op = op;
  p->flags = flags;
  if ((flags & XF_T) && info->subsampling == JDS_SS_422) {
    snprintf(msg, msg_n,
             "4:2:2 takes only hflip, vflip and rot180: a transposed 4:2:2 file has 1x2 luma sampling (4:4:0), "
             "which this library does not read");
    return JDS_ENOTSUP;
  }
  // the mirrored SOURCE axes: after a transposition the left-right mirror runs along the source's rows
  const bool mh = (flags & XF_T) ? (flags & XF_FV) != 0 : (flags & XF_FH) != 0;
  const bool mv = (flags & XF_T) ? (flags & XF_FH) != 0 : (flags & XF_FV) != 0;
  int64_t cH = info->H, cW = info->W;
  const int mw = 8 * sf.hs, mhh = 8 * sf.vs;
  if (mh && cW % mw) {
    if (!trim) {
      snprintf(msg, msg_n,
               "this operation mirrors the horizontal axis: width %lld is not a multiple of %d (JDS_XF_TRIM drops "
               "the partial MCU column)",
               (long long)cW, mw);
      return JDS_ENOTSUP;
    }
    cW -= cW % mw;
  }
  if (mv && cH % mhh) {
    if (!trim) {
      snprintf(msg, msg_n,
               "this operation mirrors the vertical axis: height %lld is not a multiple of %d (JDS_XF_TRIM drops the "
               "partial MCU row)",
               (long long)cH, mhh);
      return JDS_ENOTSUP;
    }
    cH -= cH % mhh;
  }
  if (cH < 1 || cW < 1) {
    snprintf(msg, msg_n, "trim leaves nothing of %lldx%lld", (long long)info->H, (long long)info->W);
    return JDS_EINVAL;
  }
  p->cH = cH;
  p->cW = cW;
  jds_jpeg_info crop = *info, &d = p->dst;
  d = *info;
  crop.H = cH;
  crop.W = cW;
  d.H = (flags & XF_T) ? cW : cH;
  d.W = (flags & XF_T) ? cH : cW;
  McuFile cf, df;
  d.coeffs_needed = 0;
  // a grayscale file: the MCU is one block whatever its sampling byte says (sf.hs = sf.vs = 1), every
  // operation is allowed, and components 1 and 2 keep empty grids on both sides (no tiles)
  const int ncomp = info->subsampling == JDS_SS_GRAY ? 1 : 3;
  for (int c = 0; c < ncomp; ++c) {  // the T.81 grids of both sizes
    const int64_t xcw = c ? (cW + sf.hs - 1) / sf.hs : cW, ych = c ? (cH + sf.vs - 1) / sf.vs : cH;
    const int64_t xdw = c ? (d.W + sf.hs - 1) / sf.hs : d.W, ydh = c ? (d.H + sf.vs - 1) / sf.vs : d.H;
    crop.grid_cols[c] = (xcw + 7) / 8;
    crop.grid_rows[c] = (ych + 7) / 8;
    d.grid_cols[c] = (xdw + 7) / 8;
    d.grid_rows[c] = (ydh + 7) / 8;
    d.coeffs_needed += 64 * d.grid_cols[c] * d.grid_rows[c];
  }
  d.mcu_cols = (d.W + mw - 1) / mw;
  d.mcu_rows = (d.H + mhh - 1) / mhh;
  if (mcu_file_of(&crop, &cf) || mcu_file_of(&d, &df)) {
    snprintf(msg, msg_n, "transform: no T.81 geometry for the result");
    return JDS_EINVAL;
  }
  XfFile& r = p->rec;
  r.flags = flags;
  for (int c = 0; c < 3; ++c) {
    r.sgw[c] = sf.gw[c];
    r.xr[c] = cf.gh[c];
    r.xc[c] = cf.gw[c];
    r.dgw[c] = df.gw[c];
    r.dgh[c] = df.gh[c];
    r.soff[c] = sf.off[c];
    r.doff[c] = df.off[c];
    // the grid formulas are symmetric in the two axes: block for block
    if (r.dgw[c] != ((flags & XF_T) ? r.xr[c] : r.xc[c]) || r.dgh[c] != ((flags & XF_T) ? r.xc[c] : r.xr[c]) ||
        r.xr[c] > sf.gh[c] || r.xc[c] > sf.gw[c]) {
      snprintf(msg, msg_n, "transform: the result's grids do not match the source's");
      return JDS_EINVAL;
    }
  }
  p->tiles = xf_set_tiles(&r, 0);
  return JDS_OK;
}

// ------------------------------------------------------- EXIF, prefix --

// The EXIF Orientation of a header prefix (whole marker segments, as
// mcu_splice leaves them): the first APP1 segment that starts with "Exif\0\0",
// its TIFF header (II or MM, 42, IFD0 offset), tag 0x0112 of type SHORT and
// count 1 in IFD0.  Returns 1..8 with *pos = the value's first byte in the
// prefix and *big = its byte order, or 0: no such segment, a malformed one
// (every offset is checked against the segment), no tag, a value outside 1..8.
inline int xf_exif_orientation(const uint8_t* pfx, int64_t n, int64_t* pos, int* big) {
  int64_t p = 0;
  while (p + 4 <= n && pfx[p] == 0xFF) {
    const int64_t ln = ((int64_t)pfx[p + 2] << 8) | pfx[p + 3];
    if (ln < 2 || p + 2 + ln > n) return 0;
    const uint8_t* s = pfx + p + 4;  // the segment's body
    const int64_t sn = ln - 2;
    if (pfx[p + 1] == 0xE1 && sn >= 6 && memcmp(s, "Exif\0\0", 6) == 0) {
      const uint8_t* t = s + 6;  // the TIFF header: offsets count from here
      const int64_t tn = sn - 6;
      if (tn < 8) return 0;
      bool be;
      if (t[0] == 'M' && t[1] == 'M') be = true;
      else if (t[0] == 'I' && t[1] == 'I') be = false;
      else return 0;
      auto u16 = [&](int64_t o) { return be ? (t[o] << 8) | t[o + 1] : (t[o + 1] << 8) | t[o]; };
      auto u32 = [&](int64_t o) {
        return be ? ((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | t[o + 3]
                  : ((uint32_t)t[o + 3] << 24) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 1] << 8) | t[o];
      };
      if (u16(2) != 42) return 0;
      const int64_t ifd = (int64_t)u32(4);
      if (ifd < 8 || ifd + 2 > tn) return 0;
      const int64_t cnt = u16(ifd);
      if (ifd + 2 + 12 * cnt > tn) return 0;
      for (int64_t i = 0; i < cnt; ++i) {
        const int64_t e = ifd + 2 + 12 * i;
        if (u16(e) != 0x0112) continue;
        if (u16(e + 2) != 3 || u32(e + 4) != 1u) return 0;
        const int v = u16(e + 8);
        if (v < 1 || v > 8) return 0;
        *pos = (t - pfx) + e + 8;
        *big = be ? 1 : 0;
        return v;
      }
      return 0;
    }
    p += 2 + ln;
  }
  return 0;
}

// the operation an Orientation value asks for
inline int xf_op_of_orientation(int v) {
  const int ops[9] = {JDS_XF_NONE,   JDS_XF_NONE,  JDS_XF_HFLIP,      JDS_XF_ROT180, JDS_XF_VFLIP,
                      JDS_XF_TRANSPOSE, JDS_XF_ROT90, JDS_XF_TRANSVERSE, JDS_XF_ROT270};
  return v >= 1 && v <= 8 ? ops[v] : JDS_XF_NONE;
}

inline void xf_exif_reset(uint8_t* pfx, int64_t pos, int big) {
  pfx[pos] = big ? 0 : 1;
  pfx[pos + 1] = big ? 1 : 0;
}

// The prefix of a transformed file, edited in place: SOF0 gets the output's
// size; with XF_T every 8-bit table of every DQT segment is transposed (entry
// k, in zigzag order, moves to the zigzag index of the transposed position).
// Everything else stays.  Returns 0; -1: not a sequence of whole segments; -2:
// a 16-bit table or a DQT that does not hold whole tables (refused, not
// mis-transposed); -3: no SOF0.  Never reads or writes outside [pfx, pfx + n).
inline int xf_edit_prefix(uint8_t* pfx, int64_t n, int flags, int64_t H, int64_t W) {
  uint8_t inv[64];  // row-major index -> zigzag index
  for (int k = 0; k < 64; ++k) inv[MCU_ZZ[k]] = (uint8_t)k;
  int64_t p = 0;
  bool sof = false;
  while (p < n) {
    if (p + 4 > n || pfx[p] != 0xFF) return -1;
    const int m = pfx[p + 1];
    const int64_t ln = ((int64_t)pfx[p + 2] << 8) | pfx[p + 3];
    if (ln < 2 || p + 2 + ln > n) return -1;
    uint8_t* s = pfx + p + 4;
    const int64_t sn = ln - 2;
    if (m == 0xDB && (flags & XF_T)) {
      int64_t q = 0;
      while (q < sn) {
        if (s[q] >> 4) return -2;
        if (q + 65 > sn) return -2;
        uint8_t t[64];
        memcpy(t, s + q + 1, 64);
        for (int k = 0; k < 64; ++k) {
          const int rm = MCU_ZZ[k];
          s[q + 1 + inv[8 * (rm & 7) + (rm >> 3)]] = t[k];
        }
        q += 65;
      }
    } else if (m == 0xC0) {
      if (sn < 5) return -1;
      s[1] = (uint8_t)(H >> 8);
      s[2] = (uint8_t)(H & 255);
      s[3] = (uint8_t)(W >> 8);
      s[4] = (uint8_t)(W & 255);
      sof = true;
    }
    p += 2 + ln;
  }
  return sof ? 0 : -3;
}

}  // namespace jds
