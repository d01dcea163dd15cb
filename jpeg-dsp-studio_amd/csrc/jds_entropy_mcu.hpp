// jds_entropy_mcu.hpp — what the interleaved-scan writer's kernels
// (jds_entropy_mcu.hip), its host model (jds_selftest_jpeg_transcode) and the
// stand-alone sanitizer program (tools/jpeg_splice_san.cpp) share (DESIGN.md
// "Transcode"; byte-for-byte definition: tests/transcode_ref.py): the per-file
// geometry record, the scan-order block lookup, the DC predecessor rule, the
// header splicer and the host model of the writer.  Compiles for host and
// device.  No HIP types here.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "jds.h"
#include "jds_huffopt.hpp"

#ifdef __HIPCC__
#define JDS_MCU __host__ __device__ __forceinline__
#else
#define JDS_MCU inline
#endif

namespace jds {

// One file of a batch.  The writer's scan is the file's single interleaved
// scan: blocks in MCU raster order, inside an MCU the hs x vs luma blocks in
// raster order, then Cb, then Cr (T.81 A.2.3).  Segment g of the batch's
// segment table is blocks [64 (g - seg0), 64 (g - seg0) + 64) of that scan.
struct McuFile {
  int32_t bpm;                 // blocks per MCU: hs * vs + 2; a grayscale file: 1 (the MCU is one block)
  int32_t mcu_cols, mcu_rows;
  int32_t nblk;                // bpm * mcu_cols * mcu_rows, padding blocks included
  int32_t hs, vs;              // luma sampling factors (chroma: 1 x 1)
  int32_t gw[3], gh[3];        // T.81 block grids: columns, rows
  int32_t seg0, nseg;          // its segments in the batch's table
  int32_t frame;               // its code tables (OptFrame): its own when optimised, the shared Annex K one otherwise
  int32_t pfx_len;             // header prefix: the bytes between SOI and the first DHT
  int32_t gray;                // 1: one component -- two DHT segments (0x00, 0x10) and the SOS of Ns = 1
  int32_t comp_id;             // gray: the frame's component id, which the SOS names (mcu_gray_id)
  int64_t off[3];              // a plane's first coefficient, from the coefficient base (jds_decode_jpeg's layout)
  int64_t raw_w0;              // the packed scan's first word
  int64_t raw_words;           // its capacity
  int64_t pfx_off;             // the prefix's place among the batch's prefixes
};

constexpr int MCU_SOS = 14;    // FF DA 00 0C 03 | 1 00 2 11 3 11 | 00 3F 00
constexpr int MCU_SOS1 = 10;   // grayscale: FF DA 00 08 01 | id 00 | 00 3F 00

// A scan position as (MCU column, MCU row, slot): two divisions, done once per
// block (bpm is 1, 3, 4 or 6, so the first is by a constant on every path).
struct McuPos {
  int mx, my, slot;
};
JDS_MCU McuPos mcu_pos(const McuFile& f, int n) {
  const int mcu = f.bpm == 6 ? n / 6 : (f.bpm == 4 ? n >> 2 : (f.bpm == 1 ? n : n / 3));
  McuPos p;
  p.slot = n - mcu * f.bpm;
  p.my = mcu / f.mcu_cols;
  p.mx = mcu - p.my * f.mcu_cols;
  return p;
}

// The block in slot `slot` of MCU (mx, my): its component; addr = its first
// coefficient, or -1 for a block that pads the image to whole MCUs.
JDS_MCU int mcu_slot_block(const McuFile& f, int mx, int my, int slot, long long& addr) {
  const int ny = f.hs * f.vs;
  const int c = slot < ny ? 0 : slot - ny + 1;
  const int by = c ? 0 : (f.hs == 2 ? slot >> 1 : slot), bx = c ? 0 : (f.hs == 2 ? slot & 1 : 0);  // (hs is 1 or 2)
  const int col = c ? mx : mx * f.hs + bx, row = c ? my : my * f.vs + by;
  // (selects, not f.gw[c]: on the device the record's fields are scalar loads, the component is per lane)
  const int gw = c == 0 ? f.gw[0] : (c == 1 ? f.gw[1] : f.gw[2]);
  const int gh = c == 0 ? f.gh[0] : (c == 1 ? f.gh[1] : f.gh[2]);
  const long long off = c == 0 ? f.off[0] : (c == 1 ? f.off[1] : f.off[2]);
  addr = (col < gw && row < gh) ? off + 64ll * ((long long)row * gw + col) : -1ll;
  return c;
}

// Scan position -> component and block (or padding).
JDS_MCU int mcu_locate(const McuFile& f, const McuPos& p, long long& addr) {
  return mcu_slot_block(f, p.mx, p.my, p.slot, addr);
}
JDS_MCU int mcu_locate(const McuFile& f, int n, long long& addr) { return mcu_locate(f, mcu_pos(f, n), addr); }

// The DC predecessor of the block at a scan position: the preceding block of
// its component in scan order -- the component's previous slot in this MCU, or
// its last slot in the previous MCU -- and, since a padding block repeats the
// DC before it, the nearest real block back from there: at most 2 hs vs - 1
// steps.  -1: the scan's first block of the component (prediction 0).  On T.81
// grids slot 0 of every component is real, so the walk always ends in this MCU
// or the previous one.  With one block per MCU (grayscale) that is the previous
// block in raster order.
JDS_MCU long long mcu_pred(const McuFile& f, const McuPos& p) {
  const int ny = f.hs * f.vs;
  const int lo = p.slot < ny ? 0 : p.slot, hi = p.slot < ny ? ny - 1 : p.slot;
  long long a;
  for (int j = p.slot - 1; j >= lo; --j) {
    mcu_slot_block(f, p.mx, p.my, j, a);
    if (a >= 0) return a;
  }
  if (p.mx == 0 && p.my == 0) return -1ll;
  const int qx = p.mx ? p.mx - 1 : f.mcu_cols - 1, qy = p.mx ? p.my : p.my - 1;  // the previous MCU in raster order
  for (int j = hi; j >= lo; --j) {
    mcu_slot_block(f, qx, qy, j, a);
    if (a >= 0) return a;
  }
  return -1ll;
}
JDS_MCU long long mcu_pred(const McuFile& f, int n) { return mcu_pred(f, mcu_pos(f, n)); }

// The geometry of a parsed (or caller-filled) info; seg0, frame, raw_w0 and
// the prefix fields are the batch's business.  -1: the grids are not the T.81
// grids of H x W at this subsampling, or the size is outside baseline's.
inline int mcu_file_of(const jds_jpeg_info* info, McuFile* f) {
  memset(f, 0, sizeof *f);
  const int ss = info->subsampling;
  if (ss != JDS_SS_444 && ss != JDS_SS_422 && ss != JDS_SS_420 && ss != JDS_SS_GRAY) return -1;
  const int64_t H = info->H, W = info->W;
  if (H < 1 || W < 1 || H > 65535 || W > 65535 || H * W > (int64_t)1 << 28) return -1;
  if (ss == JDS_SS_GRAY) {  // one plane, no padding blocks; components 1 and 2 are empty and start at its end
    f->hs = f->vs = f->bpm = f->gray = f->comp_id = 1;
    f->gw[0] = f->mcu_cols = (int32_t)((W + 7) / 8);
    f->gh[0] = f->mcu_rows = (int32_t)((H + 7) / 8);
    if (info->grid_cols[0] != f->gw[0] || info->grid_rows[0] != f->gh[0]) return -1;
    f->nblk = f->gw[0] * f->gh[0];
    f->off[1] = f->off[2] = 64ll * f->nblk;
    f->nseg = (f->nblk + 63) / 64;
    return 0;
  }
  f->hs = ss == JDS_SS_444 ? 1 : 2;
  f->vs = ss == JDS_SS_420 ? 2 : 1;
  f->bpm = f->hs * f->vs + 2;
  f->mcu_cols = (int32_t)((W + 8 * f->hs - 1) / (8 * f->hs));
  f->mcu_rows = (int32_t)((H + 8 * f->vs - 1) / (8 * f->vs));
  f->nblk = f->bpm * f->mcu_cols * f->mcu_rows;
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    const int64_t xc = c ? (W + f->hs - 1) / f->hs : W, yc = c ? (H + f->vs - 1) / f->vs : H;
    f->gw[c] = (int32_t)((xc + 7) / 8);
    f->gh[c] = (int32_t)((yc + 7) / 8);
    if (info->grid_cols[c] != f->gw[c] || info->grid_rows[c] != f->gh[c]) return -1;
    f->off[c] = off;
    off += 64ll * f->gw[c] * f->gh[c];
  }
  f->nseg = (f->nblk + 63) / 64;
  return 0;
}

inline int64_t mcu_coeffs(const McuFile& f) { return f.off[2] + 64ll * f.gw[2] * f.gh[2] - f.off[0]; }

// ------------------------------------------------------------ splicer --

// The header prefix of a transcoded file: every marker segment of the input
// between SOI and its first SOS, verbatim and in order, except DHT and DRI
// (fill bytes between segments are dropped).  out == nullptr: only the length.
// A grayscale file's prefix needs nothing else: its SOF0 (Nf = 1, the
// component id and sampling byte as written) travels verbatim.
// Returns the prefix's length, or -1 when the bytes are not a marker sequence
// that reaches an SOS inside [data, data + len) -- what jds_jpeg_parse rejects
// as well.  Never reads outside [data, data + len) nor writes outside
// [out, out + cap).
inline int64_t mcu_splice(const uint8_t* data, int64_t len, uint8_t* out, int64_t cap) {
  if (!data || len < 4 || data[0] != 0xFF || data[1] != 0xD8) return -1;
  int64_t p = 2, n = 0;
  for (;;) {
    if (p + 2 > len || data[p] != 0xFF) return -1;
    const int m = data[p + 1];
    if (m == 0xFF) {
      ++p;
      continue;
    }
    if (m == 0xDA) return n;
    if (m == 0xD9 || m == 0xD8 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7)) return -1;
    if (p + 4 > len) return -1;
    const int64_t ln = ((int64_t)data[p + 2] << 8) | data[p + 3];
    if (ln < 2 || p + 2 + ln > len) return -1;
    if (m != 0xC4 && m != 0xDD) {
      if (out) {
        if (n + 2 + ln > cap) return -1;
        memcpy(out + n, data + p, (size_t)(2 + ln));
      }
      n += 2 + ln;
    }
    p += 2 + ln;
  }
}

// row-major index of the k-th zigzag coefficient
constexpr uint8_t MCU_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int MCU_PFX_DEFAULT_MAX = 18 + 3 * 69 + 19;

// The component id in the SOF0 of a grayscale file's prefix (1 where the
// prefix holds no one-component SOF0: the caller's business).  Never reads
// outside [pfx, pfx + len).
inline int mcu_gray_id(const uint8_t* pfx, int64_t len) {
  int64_t p = 0;
  while (pfx && p + 4 <= len && pfx[p] == 0xFF) {
    if (pfx[p + 1] == 0xFF) {
      ++p;
      continue;
    }
    const int64_t ln = ((int64_t)pfx[p + 2] << 8) | pfx[p + 3];
    if (ln < 2 || p + 2 + ln > len) break;
    if (pfx[p + 1] == 0xC0) return ln >= 11 && pfx[p + 9] == 1 ? pfx[p + 10] : 1;
    p += 2 + ln;
  }
  return 1;
}

// What jds_encode_jpeg writes when the caller gives no prefix: APP0 (JFIF
// 1.01), one DQT per table id in use (in component order), SOF0.  out:
// MCU_PFX_DEFAULT_MAX bytes.  Returns the length, or -(1 + 64 c + i) when
// qtable[c][i] is not an integer in [1, 255], or -1000 for a table id above 3.
inline int mcu_default_prefix(const jds_jpeg_info* info, uint8_t* out) {
  int p = 0;
  const uint8_t app0[18] = {0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  memcpy(out, app0, 18);
  p = 18;
  bool done[4] = {false, false, false, false};
  const int ncomp = info->subsampling == JDS_SS_GRAY ? 1 : 3;  // (a grayscale info's tq[1..2] are not read)
  for (int c = 0; c < ncomp; ++c) {
    const int id = info->tq[c];
    if (id < 0 || id > 3) return -1000;
    if (done[id]) continue;
    done[id] = true;
    const uint8_t h[5] = {0xFF, 0xDB, 0x00, 0x43, (uint8_t)id};
    memcpy(out + p, h, 5);
    p += 5;
    for (int k = 0; k < 64; ++k) {
      const double v = info->qtable[c][MCU_ZZ[k]];
      if (!(v >= 1.0 && v <= 255.0) || v != (double)(int)v) return -(1 + 64 * c + MCU_ZZ[k]);
      out[p++] = (uint8_t)(int)v;
    }
  }
  const int H = (int)info->H, W = (int)info->W;
  if (ncomp == 1) {  // Nf = 1, id 1, sampling 0x11
    const uint8_t sof[13] = {0xFF, 0xC0, 0x00, 0x0B, 0x08, (uint8_t)(H >> 8), (uint8_t)(H & 255), (uint8_t)(W >> 8),
                             (uint8_t)(W & 255), 1, 1, 0x11, (uint8_t)info->tq[0]};
    memcpy(out + p, sof, 13);
    return p + 13;
  }
  const int smp = info->subsampling == JDS_SS_420 ? 0x22 : (info->subsampling == JDS_SS_422 ? 0x21 : 0x11);
  const uint8_t sof[19] = {0xFF, 0xC0, 0x00, 0x11, 0x08, (uint8_t)(H >> 8), (uint8_t)(H & 255), (uint8_t)(W >> 8),
                           (uint8_t)(W & 255), 3, 1, (uint8_t)smp, (uint8_t)info->tq[0], 2, 0x11, (uint8_t)info->tq[1],
                           3, 0x11, (uint8_t)info->tq[2]};
  memcpy(out + p, sof, 19);
  return p + 19;
}

// --------------------------------------------------------- host model --

// The Annex K tables: DC luma, AC luma, DC chroma, AC chroma (the DHT order)
struct McuStdTabs {
  const uint8_t* bits[4];
  const uint8_t* vals[4];
  int n_vals[4];
};

struct McuHostTab {
  uint8_t bits[16];
  uint8_t vals[256];
  int n_vals;
  uint32_t code[256];  // symbol -> length << 16 | code
};

inline void mcu_host_codes(McuHostTab* t) {
  memset(t->code, 0, sizeof t->code);
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < t->bits[len - 1]; ++i, ++k) t->code[t->vals[k]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
}

// A block's symbols through `sym(is_dc, symbol, magnitude bits, their count)`
// in stream order, with the coder's clamps (DC category 11, AC category 10);
// returns whether the block is baseline-codable.
template <class F>
inline bool mcu_host_block(const int16_t* blk, int pred, F&& sym) {
  bool ok = true;
  const int dc = blk ? blk[0] : pred;
  const int diff = dc - pred;
  auto cat = [](int v) {
    int a = v < 0 ? -v : v, s = 0;
    while (a) {
      ++s;
      a >>= 1;
    }
    return s;
  };
  int ds = cat(diff);
  if (ds > 11) {
    ok = false;
    ds = 11;
  }
  sym(true, ds, (uint32_t)(diff + (diff >> 31)) & ((1u << ds) - 1u), ds);
  int last = 0;
  if (blk)
    for (int k = 1; k < 64; ++k) {
      const int v = blk[MCU_ZZ[k]];
      if (!v) continue;
      int run = k - 1 - last;
      for (; run >= 16; run -= 16) sym(false, 0xF0, 0u, 0);
      int s = cat(v);
      if (s > 10) {
        ok = false;
        s = 10;
      }
      sym(false, (run << 4) | s, (uint32_t)(v + (v >> 31)) & ((1u << s) - 1u), s);
      last = k;
    }
  if (last < 63) sym(false, 0x00, 0u, 0);
  return ok;
}

// The writer on the host, block by block in scan order through the kernels'
// own lookup (mcu_locate), predecessor rule (mcu_pred) and table builder
// (ho_build_host), a serial bit writer standing in for the lanes' staging and
// placement.  coeffs: the file's planes (f.off from 0).  Returns 0, or 1 when a
// block is not baseline-codable (out is left empty).
inline int mcu_host_write(const McuFile& f, const int16_t* coeffs, int optimize, const uint8_t* pfx, int64_t pfx_len,
                          const McuStdTabs& std_tabs, std::vector<uint8_t>* out) {
  out->clear();
  McuHostTab tab[4];
  for (int t = 0; t < 4; ++t) {
    memset(&tab[t], 0, sizeof tab[t]);
    memcpy(tab[t].bits, std_tabs.bits[t], 16);
    memcpy(tab[t].vals, std_tabs.vals[t], (size_t)std_tabs.n_vals[t]);
    tab[t].n_vals = std_tabs.n_vals[t];
  }
  bool ok = true;
  auto each_block = [&](auto&& sym) {
    for (int n = 0; n < f.nblk; ++n) {
      long long a;
      const int c = mcu_locate(f, n, a);
      const long long pa = mcu_pred(f, n);
      const int pred = pa >= 0 ? coeffs[pa] : 0;
      // a padding block repeats the DC before it: its predecessor's, through the same walk
      ok = mcu_host_block(a >= 0 ? coeffs + a : nullptr, pred, [&](bool dc, int s, uint32_t mag, int ml) {
             sym(c ? 1 : 0, dc, s, mag, ml);
           }) && ok;
    }
  };
  const int ntab = f.gray ? 2 : 4;  // a grayscale file: the luma class alone
  if (optimize) {
    std::vector<uint32_t> freq(4 * 256, 0u);
    each_block([&](int cls, bool dc, int s, uint32_t, int) { freq[(size_t)(2 * cls + (dc ? 0 : 1)) * 256 + s]++; });
    for (int t = 0; t < ntab; ++t) {
      HoTable ht;
      ho_build_host(&freq[(size_t)t * 256], &ht);
      if (ht.fell_back) continue;
      memcpy(tab[t].bits, ht.bits, 16);
      memcpy(tab[t].vals, ht.vals, 256);
      tab[t].n_vals = ht.n_vals;
    }
  }
  for (int t = 0; t < 4; ++t) mcu_host_codes(&tab[t]);
  std::vector<uint8_t>& o = *out;
  o.push_back(0xFF);
  o.push_back(0xD8);
  o.insert(o.end(), pfx, pfx + pfx_len);
  const int tc_th[4] = {0x00, 0x10, 0x01, 0x11};
  for (int t = 0; t < ntab; ++t) {
    const int len = 3 + 16 + tab[t].n_vals;
    const uint8_t h[5] = {0xFF, 0xC4, (uint8_t)(len >> 8), (uint8_t)(len & 255), (uint8_t)tc_th[t]};
    o.insert(o.end(), h, h + 5);
    o.insert(o.end(), tab[t].bits, tab[t].bits + 16);
    o.insert(o.end(), tab[t].vals, tab[t].vals + tab[t].n_vals);
  }
  const uint8_t sos[MCU_SOS] = {0xFF, 0xDA, 0x00, 0x0C, 0x03, 1, 0x00, 2, 0x11, 3, 0x11, 0x00, 0x3F, 0x00};
  const uint8_t sos1[MCU_SOS1] = {0xFF, 0xDA, 0x00, 0x08, 0x01, (uint8_t)mcu_gray_id(pfx, pfx_len), 0x00, 0x00, 0x3F, 0x00};
  if (f.gray)
    o.insert(o.end(), sos1, sos1 + MCU_SOS1);
  else
    o.insert(o.end(), sos, sos + MCU_SOS);
  uint64_t acc = 0;
  int nacc = 0;
  auto put = [&](uint32_t v, int n) {
    if (!n) return;
    acc = (acc << n) | (v & ((1ull << n) - 1ull));
    nacc += n;
    while (nacc >= 8) {
      nacc -= 8;
      const uint8_t b = (uint8_t)(acc >> nacc);
      o.push_back(b);
      if (b == 0xFF) o.push_back(0x00);
    }
  };
  ok = true;
  each_block([&](int cls, bool dc, int s, uint32_t mag, int ml) {
    const uint32_t e = tab[2 * cls + (dc ? 0 : 1)].code[s];
    put(e & 0xFFFFu, (int)(e >> 16));
    put(mag, ml);
  });
  if (nacc) put((1u << (8 - nacc)) - 1u, 8 - nacc);
  o.push_back(0xFF);
  o.push_back(0xD9);
  if (!ok) {
    out->clear();
    return 1;
  }
  return 0;
}

}  // namespace jds
