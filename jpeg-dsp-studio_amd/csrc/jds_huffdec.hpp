// jds_huffdec.hpp — baseline JFIF parsing and the Huffman decode core of the
// self-synchronising entropy decoder (jds_entropy_dec.hip; DESIGN.md "Entropy
// decode").  Compiles for host and device: the GPU lanes, the host model behind
// jds_selftest_huffdec and the stand-alone sanitizer program
// (tools/jfif_host_san.cpp) run this same code.  No HIP types here.  Scans
// with restart intervals (DRI) decode one interval per lane (hd_rst_lane).
//
// Stream positions are bit positions in the STUFFED scan bytes: the reader
// skips the 0x00 after every 0xFF itself, so a position never points into a
// stuffed byte.  A decoder state is (p, k, slot): p the position of the next
// symbol, k the zigzag index it belongs to (0: a DC symbol is expected), slot
// the block's index within its MCU (always 0 in a non-interleaved scan, whose
// MCU is one block), packed as p << 16 | slot << 8 | k.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jds.h"

#ifdef __HIPCC__
#define JDS_HDI __host__ __device__ __forceinline__
#else
#define JDS_HDI inline
#endif

namespace jds {

constexpr uint64_t HD_NONE = ~0ull;  // "no state": an invalid decode publishes nothing

// frame status bits (include/jds.h JDS_DEC_*)
enum : uint32_t {
  HD_BAD_HEADER = JDS_DEC_HEADER,
  HD_BAD_CODE = JDS_DEC_CODE,
  HD_K63 = JDS_DEC_K63,
  HD_OVERRUN = JDS_DEC_OVERRUN,
  HD_COUNT = JDS_DEC_COUNT,
  HD_DC_RANGE = JDS_DEC_DC_RANGE,
  HD_RESTART = JDS_DEC_RESTART
};

// Decode table of one Huffman table: codes of up to 8 bits resolve through
// lut[next 8 bits] = length << 8 | symbol (0: longer code); longer ones by the
// canonical-code compare: the smallest length l in 9..16 with
// v16 < limit[l - 9] (the left-aligned end of the codes of length <= l), then
// vals[offs[l - 9] + (v16 >> (16 - l))].
struct HuffDecTab {
  uint16_t lut[256];
  uint32_t limit[8];
  int32_t offs[8];
  uint8_t vals[256];
};

// T.81 Annex C from BITS / HUFFVAL.  -1: the lengths over-subscribe the code
// space or name more than 256 symbols.
inline int hd_build(const uint8_t* bits, const uint8_t* vals, HuffDecTab* t) {
  memset(t, 0, sizeof *t);
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    const uint32_t first = code, cnt = bits[l - 1];
    if (first + cnt > (1u << l) || k + (int)cnt > 256) return -1;
    if (l <= 8)
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t c = first + i;
        for (uint32_t j = 0; j < (1u << (8 - l)); ++j)
          t->lut[(c << (8 - l)) + j] = (uint16_t)((l << 8) | vals[k + i]);
      }
    code = first + cnt;
    k += (int)cnt;
    if (l >= 9) {
      t->limit[l - 9] = code << (16 - l);
      t->offs[l - 9] = (k - (int)cnt) - (int)first;
    }
    code <<= 1;
  }
  memcpy(t->vals, vals, (size_t)k);
  return k;
}

JDS_HDI uint64_t hd_pack(uint64_t p, int k, int slot = 0) {
  return (p << 16) | ((uint64_t)(uint32_t)slot << 8) | (uint64_t)(uint32_t)k;
}

// The MCU of an interleaved scan (T.81 A.2.3) and the frame's block grids
// (host-built; the kernels keep a copy in LDS).  Components come in frame
// order, so a component's hs * vs slots are consecutive from first[c], in
// raster order inside the MCU.  A block whose grid coordinates
// (mx * hs + bx, my * vs + by) lie outside its component's T.81 grid pads the
// image to whole MCUs: it is decoded, its DC difference counts in the
// component's prediction, and it is not stored.
struct HdMcu {
  int32_t bpm;                 // blocks per MCU: 6 (4:2:0), 4 (4:2:2), 3 (4:4:4)
  int32_t mcu_cols, mcu_rows;
  int32_t hs[3], vs[3];        // sampling factors
  int32_t gw[3], gh[3];        // T.81 block grid: columns, rows
  int32_t first[3];            // a component's first slot
  int64_t off[3];              // the first coefficient of a component's plane, from the coeffs base
  uint8_t comp[8], bx[8], by[8];  // per slot
  uint8_t dct[8], act[8];         // per slot: DC / AC table, indices into the four-table array
};

// Table choice per symbol.  HdPlain: one DC and one AC table, no slot (a
// non-interleaved scan).  HdIl: by slot, from the MCU descriptor.
struct HdPlain {
  static constexpr bool IL = false;
  const HuffDecTab *dc, *ac;
  JDS_HDI const HuffDecTab* tab(bool isdc, int) const { return isdc ? dc : ac; }
  JDS_HDI int next(int slot) const { return slot; }
  JDS_HDI int slot_of(int64_t) const { return 0; }
};
struct HdIl {
  static constexpr bool IL = true;
  const HuffDecTab* tabs;  // [0] DC 0, [1] DC 1, [2] AC 0, [3] AC 1
  const HdMcu* m;
  JDS_HDI const HuffDecTab* tab(bool isdc, int slot) const { return tabs + (isdc ? m->dct[slot] : m->act[slot]); }
  JDS_HDI int next(int slot) const { return slot + 1 == m->bpm ? 0 : slot + 1; }
  JDS_HDI int slot_of(int64_t blk) const { return (int)(blk % m->bpm); }
};

// A scan's stuffed bytes as the decode reads them.  A source has the scan's
// length n, byte(i) for 0 <= i < n, and bytes10(b, lo, hi): the bytes b .. b+9
// (b >= 0), little-endian in lo (b .. b+7) and hi (b+8, b+9); what lies at or
// past n is unspecified there (hd_window masks it) but is never read from
// outside the scan.  HdMemSrc reads memory directly (host model; the kernels
// stage a workgroup's bytes in LDS, jds_entropy_dec.hip).
struct HdMemSrc {
  const uint8_t* d;
  int64_t n;
  JDS_HDI uint32_t byte(int64_t i) const { return d[i]; }
  JDS_HDI void bytes10(int64_t b, uint64_t& lo, uint64_t& hi) const {
    lo = 0;
    hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (b + j < n) lo |= (uint64_t)d[b + j] << (8 * j);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (b + 8 + j < n) hi |= (uint64_t)d[b + 8 + j] << (8 * j);
  }
};

// The guess a subsequence starts from: its first bit, a DC symbol expected.
// A first byte that is the stuffed 0x00 of the previous subsequence's last
// 0xFF is skipped.
template <class Src>
JDS_HDI uint64_t hd_guess(const Src& src, int64_t first_bit) {
  const int64_t b = first_bit >> 3;
  uint64_t p = (uint64_t)first_bit;
  if ((first_bit & 7) == 0 && b > 0 && b < src.n && src.byte(b) == 0x00 && src.byte(b - 1) == 0xFF) p += 8;
  return hd_pack(p, 0);
}

// The next five data bytes from byte b on (40 bits in w, first byte on top)
// and, per data byte, whether a stuffed byte follows it (ffm bit j).  Bytes
// at or past n read as 0xFF data.  The first eight raw bytes are taken
// big-endian into one word; every in-range 0xFF among the data bytes is found
// at once (exact zero-byte test on the complement) and the byte after it
// squeezed out, at most three times (most windows hold none, and a wave pays
// one step when any of its lanes holds one).  A window with more stuffed
// bytes than eight raw bytes cover takes the byte-by-byte walk below.
// Nothing here is indexed at run time.
template <class Src>
JDS_HDI void hd_window(const Src& src, int64_t b, uint64_t& w, uint32_t& ffm) {
  uint64_t lo, hi;
  src.bytes10(b, lo, hi);
  const int64_t left = src.n - b;  // bytes of the scan from b on (>= 1)
  const uint64_t valid = left >= 8 ? ~0ull : ~(~0ull >> (8 * (int)left));  // the in-range bytes, from the top
  uint64_t V = __builtin_bswap64(lo) | ~valid;
  const uint64_t L7 = 0x7F7F7F7F7F7F7F7Full, inv = ~V;
  uint64_t ff = ~(((inv & L7) + L7) | inv | L7) & valid;  // 0x80 in every in-range byte that is 0xFF
  ffm = 0;
  for (int s = 0; s < 3 && (ff >> 24); ++s) {  // an 0xFF among data bytes 0..4
    const int i = __builtin_clzll(ff) >> 3;   // the first one, counted from the top
    const uint64_t keep = ~0ull << (8 * (7 - i));  // bytes 0..i stay
    ffm |= 1u << i;
    V = (V & keep) | ((V << 8) & ~keep);
    ff = ((ff & keep) | ((ff << 8) & ~keep)) & ~(0x80ull << (8 * (7 - i)));
  }
  if (!(ff >> 24)) {
    w = V >> 24;
    return;
  }
  uint32_t x[10];
#pragma unroll
  for (int j = 0; j < 10; ++j)
    x[j] = j < left ? (uint32_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFFu) : 0x100u;
  w = 0;
  ffm = 0;
  int cnt = 0;
  bool skip = false;
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    const bool take = !skip && cnt < 5;
    skip = take && x[j] == 0xFFu;  // in range and 0xFF: the next byte is its stuffing
    if (take) {
      w = (w << 8) | (x[j] & 0xFFu) | (x[j] >> 8) * 0xFFu;
      if (skip) ffm |= 1u << cnt;
      ++cnt;
    }
  }
}

struct HdNullSink {
  JDS_HDI void operator()(int64_t, int, int) const {}
};

// Decode from (p, k, slot) while p < pend and blk < blk_end: one symbol per
// iteration, DC and AC through the same body, the tables chosen by tc (per
// slot in an interleaved scan; the slot advances at every block end).
// sink(blk, k, value) receives every coefficient (the DC entry is the
// difference).  Returns the defect bits met (the decode stops there).  Reads
// are bounded by the source's scan.
template <class TC, class Src, class Sink>
JDS_HDI uint32_t hd_run(const Src& src, const TC& tc, uint64_t& p, int& k, int& slot, uint64_t pend, int64_t& blk,
                        int64_t blk_end, Sink&& sink) {
  const uint64_t nbits = (uint64_t)src.n * 8u;
  while (p < pend && p < nbits && blk < blk_end) {
    uint64_t w;
    uint32_t ffm;
    hd_window(src, (int64_t)(p >> 3), w, ffm);
    const uint32_t off = (uint32_t)(p & 7u);
    const uint32_t x = (uint32_t)((w << (24u + off)) >> 32);  // the next 32 bits
    const uint32_t v = x >> 16;
    const bool isdc = k == 0;
    const HuffDecTab* t = tc.tab(isdc, slot);
    uint32_t len = 0, sym = 0;
    const uint32_t e = t->lut[v >> 8];
    if (e) {
      len = e >> 8;
      sym = e & 255u;
    } else {
#pragma unroll
      for (int l = 9; l <= 16; ++l)
        if (!len && v < t->limit[l - 9]) {
          len = (uint32_t)l;
          sym = t->vals[(uint32_t)(t->offs[l - 9] + (int32_t)(v >> (16 - l))) & 255u];
        }
      if (!len) return HD_BAD_CODE;
    }
    const uint32_t size = isdc ? sym : (sym & 15u), run = isdc ? 0u : (sym >> 4);
    if (size > (isdc ? 11u : 10u)) return HD_BAD_CODE;  // outside baseline (or a wrong-state decode)
    int val = 0;
    if (size) {
      const uint32_t mag = (x << len) >> (32u - size);
      val = mag < (1u << (size - 1)) ? (int)mag - (int)(1u << size) + 1 : (int)mag;
    }
    if (isdc) {
      sink(blk, 0, val);
      k = 1;
    } else if (size == 0) {
      if (run == 15) {
        k += 16;
        if (k > 63) return HD_K63;
      } else {  // EOB
        k = 0;
        ++blk;
        slot = tc.next(slot);
      }
    } else {
      k += (int)run;
      if (k > 63) return HD_K63;
      sink(blk, k, val);
      if (++k == 64) {
        k = 0;
        ++blk;
        slot = tc.next(slot);
      }
    }
    const uint32_t used = len + size, nb = (off + used) >> 3;  // whole data bytes left behind (<= 4)
    p += used + 8u * (uint32_t)__builtin_popcount(ffm & ((1u << nb) - 1u));
    if (p > nbits) return HD_OVERRUN;
  }
  return 0;
}

// Synchronisation pass of one subsequence: decode from `entry` to the
// subsequence's end; returns the exit state (HD_NONE after an invalid decode)
// and the blocks completed.
template <class TC, class Src>
JDS_HDI uint64_t hd_sync_lane(const Src& src, const TC& tc, uint64_t entry, uint64_t pend, uint32_t& nblk) {
  uint64_t p = entry >> 16;
  int k = (int)(entry & 255u), slot = (int)((entry >> 8) & 255u);
  int64_t blk = 0;
  const uint32_t fl = hd_run(src, tc, p, k, slot, pend, blk, (int64_t)1 << 62, HdNullSink());
  nblk = (uint32_t)blk;
  return (fl & (HD_BAD_CODE | HD_K63)) ? HD_NONE : hd_pack(p, k, slot);
}

// The blocks are complete at position p: what follows must be the final data
// byte's pad bits (p lies inside the source's last data byte or at its end).
template <class Src>
JDS_HDI bool hd_tail_ok(const Src& src, uint64_t p) {
  const int64_t n = src.n;
  int64_t L = n - 1;
  if (n >= 2 && src.byte(n - 1) == 0x00 && src.byte(n - 2) == 0xFF) L = n - 2;
  return (int64_t)p > 8 * L && (int64_t)p <= 8 * n;
}

// One restart interval, a stream of its own (T.81 E.1.4): decode from state
// (0, 0, 0) over the interval's stuffed bytes, nblk blocks to the sink from block
// blk0 on (the sink sums the DC differences from 0 itself).  Judged alone: the
// interval must hold exactly its blocks and end in its pad bits.  The GPU lane
// (k_dec_rst) and the host model run this.  An interleaved scan's interval is
// whole MCUs, so blk0 is a first slot.
template <class TC, class Src, class Sink>
JDS_HDI uint32_t hd_rst_lane(const Src& src, const TC& tc, int64_t blk0, int64_t nblk, Sink&& sink) {
  uint64_t p = 0;
  int k = 0, slot = 0;
  int64_t blk = blk0;
  const uint32_t fl = hd_run(src, tc, p, k, slot, (uint64_t)src.n * 8u, blk, blk0 + nblk, sink);
  if (fl) return fl;
  if (blk != blk0 + nblk) return HD_COUNT;
  return hd_tail_ok(src, p) ? 0u : (uint32_t)HD_COUNT;
}

// Write pass of one subsequence, from its settled entry state and first block
// index; judges the scan: defects of the decode, data after the last block,
// or too few blocks (reported by the scan's last subsequence).  In an
// interleaved scan the settled entry's slot must be the first block's place in
// its MCU; in a defective scan it may not be (HD_COUNT).
template <class TC, class Src, class Sink>
JDS_HDI uint32_t hd_write_lane(const Src& src, const TC& tc, uint64_t entry, uint64_t pend, int64_t blk0,
                               int64_t nblocks, bool last, Sink&& sink) {
  if (entry == HD_NONE) return last ? HD_COUNT : 0;
  if (blk0 >= nblocks) return 0;
  uint64_t p = entry >> 16;
  int k = (int)(entry & 255u), slot = (int)((entry >> 8) & 255u);
  if (TC::IL && slot != tc.slot_of(blk0)) return HD_COUNT;
  int64_t blk = blk0;
  uint32_t fl = hd_run(src, tc, p, k, slot, pend, blk, nblocks, sink);
  if (fl) return fl;
  if (blk == nblocks) {
    // the scan is complete: what follows must be the final data byte's pad bits
    if (!hd_tail_ok(src, p)) fl |= HD_COUNT;
  } else if (last) {
    fl |= HD_COUNT;
  }
  return fl;
}

// One scan of one frame (host-built, jds_dec_jobs.hpp).  A launch serves descriptors
// of different files (jds_jpeg_batch_to_rgb): `file` selects the file's four
// decode tables (tabs + 4 * file) and, interleaved, its MCU descriptor
// (mcu + file), whose off[] then include the file's place in the batch's
// coefficient buffer; a non-interleaved descriptor's dc_tab / ac_tab already
// index the whole table array.  Single-file calls and plans leave file at 0.
struct DecScan {
  long long data_off;  // the scan's stuffed bytes, from the files base
  long long nbytes;
  long long coef_off;  // the scan's first coefficient, from the coeffs base
  long long dcs_off;   // interleaved: the file's first entry in the DC staging array
  int nblocks;
  int frame;
  int dc_tab, ac_tab;  // indices into the table array
  int grp0, ngrp;      // its workgroups
  int nsub;            // its subsequences
  int blk_base;        // interleaved: its first block's index in the scan's block order (whole MCUs); else 0
  int file;            // table set (and MCU descriptor) of the descriptor's file
};

// The descriptors of one instantiation of the decode kernels (dec_run_groups):
// laid out by dec_layout; scratch: dec_scratch_bytes(ngroups, nscans) device bytes.
struct DecGroup {
  const DecScan* sc;
  int nscans;
  long long ngroups;
  int max_ngrp;
  void* scratch;
  bool il;  // interleaved scans: the <true> instantiations
};

// One restart interval of one frame (k_dec_rst): built on the host for a
// parsed file, on the device (k_rst_scan) for a plan's batch.  nblk == 0: not
// decoded (its frame is skipped).  A workgroup of k_dec_rst stages one table set:
// the RST_G intervals of a workgroup belong to one file (the first one's `file`;
// a batch pads each file's intervals to whole workgroups with nblk == 0 entries).
struct RstIv {
  long long data_off;  // the interval's stuffed bytes, from the files base
  long long coef_off;  // its first block's first coefficient, from the coeffs base (interleaved: its first
                       // block's index in the scan's block order)
  int nbytes;
  int nblk;
  int frame;
  int tabs;  // dc table index | ac table index << 8 (into the file's four tables)
  int file;  // table set (tabs + 4 * file) and, interleaved, MCU descriptor (mcu + file)
  int pad_;
};

// What a plan knows about its restart files before it sees them.
struct RstGeo {
  int ri;           // the interval, in blocks
  int nblk[3];      // blocks of the Y, Cb, Cr scans
  int first[4];     // first interval of each scan within the frame; first[3]: intervals per frame
  long long off[3];  // the scans' first coefficient within the frame
  long long cpf;     // coefficients per frame
};

// Where a block of an interleaved scan goes.  n: its index in the scan's block
// order.  -> the component, and the block's first coefficient in the planar
// layout (Y, Cb, Cr; each component's T.81 grid in raster order), or null for
// a block that pads the image to whole MCUs.
JDS_HDI int16_t* hd_il_place(const HdMcu* m, int16_t* coeffs, int64_t n, int& c) {
  const int64_t mcu = n / m->bpm;
  const int slot = (int)(n - mcu * m->bpm);
  const int my = (int)(mcu / m->mcu_cols), mx = (int)(mcu - (int64_t)my * m->mcu_cols);
  c = m->comp[slot];
  const int gx = mx * m->hs[c] + m->bx[slot], gy = my * m->vs[c] + m->by[slot];
  if (gx >= m->gw[c] || gy >= m->gh[c]) return nullptr;
  return coeffs + m->off[c] + 64 * ((int64_t)gy * m->gw[c] + gx);
}

// Write pass of an interleaved scan: AC coefficients to their planar place
// (dropped for padding), every DC difference, padding included, to the staging
// array in scan order (the per-component sums run over it afterwards).  base:
// the scan-order index of the descriptor's block 0.
struct HdIlSink {
  const HdMcu* m;
  int16_t* coeffs;
  int16_t* dcs;
  const uint8_t* zz;
  int64_t base;
  int64_t cur = -1;
  int16_t* dst = nullptr;
  JDS_HDI void operator()(int64_t blk, int k, int v) {
    if (k == 0) {
      dcs[base + blk] = (int16_t)v;
      return;
    }
    if (blk != cur) {
      int c;
      cur = blk;
      dst = hd_il_place(m, coeffs, base + blk, c);
    }
    if (dst) dst[zz[k]] = (int16_t)v;
  }
};

// One restart interval of an interleaved scan, decoded by one lane: three
// running DC sums from 0 (padding blocks count), judged against int16; kept
// blocks go to their planar place.
struct HdIlRstSink {
  const HdMcu* m;
  int16_t* coeffs;
  const uint8_t* zz;
  int64_t base;
  int64_t cur = -1;
  int16_t* dst = nullptr;
  int c = 0;
  int acc0 = 0, acc1 = 0, acc2 = 0;
  bool bad = false;
  JDS_HDI void operator()(int64_t blk, int k, int v) {
    if (blk != cur) {
      cur = blk;
      dst = hd_il_place(m, coeffs, base + blk, c);
    }
    if (k == 0) {
      const int a = (c == 0 ? acc0 : (c == 1 ? acc1 : acc2)) + v;
      acc0 = c == 0 ? a : acc0;
      acc1 = c == 1 ? a : acc1;
      acc2 = c == 2 ? a : acc2;
      bad = bad || a < -32768 || a > 32767;
      v = a;
    }
    if (dst) dst[zz[k]] = (int16_t)v;
  }
};

// ------------------------------------------------------------- host side --

static const uint8_t HD_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                  58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline int hd_fail(char* msg, size_t cap, int code, const char* fmt, ...) {
  if (msg && cap) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, cap, fmt, ap);
    va_end(ap);
  }
  return code;
}

// Block counts of the reference's planes (floor-sized chroma) for a baseline
// frame; JDS_ENOTSUP where T.81's ceil-sized chroma gives another block grid
// (mirrors ent_prepare, jds_abi.hip).
inline int hd_block_counts(int64_t H, int64_t W, int mode, int64_t* ny, int64_t* nc, char* msg, size_t cap) {
  const int64_t sy = mode == JDS_SS_420 ? 2 : 1, sx = mode == JDS_SS_444 ? 1 : 2;
  const int64_t hc = H / sy, wc = W / sx;
  if (hc < 1 || wc < 1) return hd_fail(msg, cap, JDS_ENOTSUP, "%lldx%lld: empty subsampled chroma plane", (long long)H, (long long)W);
  const int64_t ncy = (hc + 7) / 8, ncx = (wc + 7) / 8;
  const int64_t jh = (H + sy - 1) / sy, jw = (W + sx - 1) / sx;
  if ((jh + 7) / 8 != ncy || (jw + 7) / 8 != ncx)
    return hd_fail(msg, cap, JDS_ENOTSUP, "%lldx%lld: the chroma block grid (%lldx%lld) differs from baseline JPEG's (%lldx%lld)",
                   (long long)H, (long long)W, (long long)ncy, (long long)ncx, (long long)((jh + 7) / 8),
                   (long long)((jw + 7) / 8));
  *ny = ((H + 7) / 8) * ((W + 7) / 8);
  *nc = ncy * ncx;
  return JDS_OK;
}

// Parse a baseline JFIF of the profile this library writes (include/jds.h:
// jds_jfif_parse), with or without restart intervals.  headers_only: stop without error where the data ends once
// SOF0 and the four Huffman tables are known (the plan's header template).
// Never reads outside [data, data + len).
inline int hd_parse(const uint8_t* data, int64_t len, jds_jfif_info* out, bool headers_only, char* msg, size_t cap) {
  if (!data || !out || len < 0) return hd_fail(msg, cap, JDS_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) return hd_fail(msg, cap, JDS_EINVAL, "not a JPEG file: SOI missing");
  uint8_t qt[4][64];
  bool qdef[4] = {false, false, false, false};
  int tq = -1;
  bool sof = false, seen[4] = {false, false, false, false};
  int ri = 0;  // the restart interval in effect (DRI), 0: none
  int64_t p = 2;
  for (;;) {
    if (p + 2 > len) {
      if (headers_only && sof) break;
      return hd_fail(msg, cap, JDS_EINVAL, "truncated file: EOI missing");
    }
    if (data[p] != 0xFF) return hd_fail(msg, cap, JDS_EINVAL, "marker expected at byte %lld", (long long)p);
    const int m = data[p + 1];
    if (m == 0xFF) {  // fill byte
      ++p;
      continue;
    }
    if (m == 0xD9) break;  // EOI
    if (m >= 0xD0 && m <= 0xD7)
      return hd_fail(msg, cap, JDS_EINVAL, "restart marker RST%d outside scan data at byte %lld", m - 0xD0, (long long)p);
    if (m == 0xD8 || m == 0x01 || m == 0x00)
      return hd_fail(msg, cap, JDS_EINVAL, "unexpected marker 0x%02X at byte %lld", m, (long long)p);
    if (p + 4 > len) return hd_fail(msg, cap, JDS_EINVAL, "truncated segment header at byte %lld", (long long)p);
    const int64_t ln = ((int64_t)data[p + 2] << 8) | data[p + 3];
    if (ln < 2 || p + 2 + ln > len)
      return hd_fail(msg, cap, JDS_EINVAL, "segment 0x%02X at byte %lld: length %lld reaches past the end of the file", m,
                     (long long)p, (long long)ln);
    const uint8_t* s = data + p + 4;
    const int64_t sl = ln - 2;
    if (m == 0xC0) {
      if (sof) return hd_fail(msg, cap, JDS_EINVAL, "second SOF0");
      if (sl < 6) return hd_fail(msg, cap, JDS_EINVAL, "SOF0 too short");
      if (s[0] != 8) return hd_fail(msg, cap, JDS_ENOTSUP, "sample precision %d (12-bit and other depths are not supported)", s[0]);
      out->H = (s[1] << 8) | s[2];
      out->W = (s[3] << 8) | s[4];
      const int nf = s[5];
      if (nf == 1) return hd_fail(msg, cap, JDS_ENOTSUP, "grayscale files (one component) are not supported");
      if (nf != 3) return hd_fail(msg, cap, JDS_ENOTSUP, "%d components (three are supported)", nf);
      if (sl != 6 + 3 * nf) return hd_fail(msg, cap, JDS_EINVAL, "SOF0 length does not match its component count");
      if (out->H < 1 || out->W < 1) return hd_fail(msg, cap, JDS_ENOTSUP, "frame size %lldx%lld (DNL is not supported)", (long long)out->H, (long long)out->W);
      for (int c = 0; c < 3; ++c)
        if (s[6 + 3 * c] != c + 1) return hd_fail(msg, cap, JDS_ENOTSUP, "component ids other than 1, 2, 3");
      const int ys = s[7];
      if (ys != 0x11 && ys != 0x21 && ys != 0x22)
        return hd_fail(msg, cap, JDS_ENOTSUP, "luma sampling %dx%d (1x1, 2x1 and 2x2 are supported)", ys >> 4, ys & 15);
      if (s[10] != 0x11 || s[13] != 0x11) return hd_fail(msg, cap, JDS_ENOTSUP, "subsampled or oversampled chroma factors");
      out->subsampling = ys == 0x11 ? JDS_SS_444 : (ys == 0x21 ? JDS_SS_422 : JDS_SS_420);
      if (s[8] != s[11] || s[8] != s[14])
        return hd_fail(msg, cap, JDS_ENOTSUP, "two quantisation tables in use (one is supported)");
      tq = s[8];
      if (tq > 3) return hd_fail(msg, cap, JDS_EINVAL, "quantisation table id %d", tq);
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8) {
      if (m == 0xCC || m >= 0xC9) return hd_fail(msg, cap, JDS_ENOTSUP, "arithmetic coding (marker 0x%02X) is not supported", m);
      return hd_fail(msg, cap, JDS_ENOTSUP, "%s (SOF%d) is not supported: baseline SOF0 only", m == 0xC2 ? "progressive JPEG" : "this frame type", m - 0xC0);
    } else if (m == 0xDD) {
      if (ln != 4) return hd_fail(msg, cap, JDS_EINVAL, "DRI segment of length %lld (4 expected)", (long long)ln);
      ri = (s[0] << 8) | s[1];
    } else if (m == 0xDB) {
      int64_t q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, id = s[q] & 15;
        if (pq == 1) return hd_fail(msg, cap, JDS_ENOTSUP, "16-bit DQT is not supported");
        if (pq != 0 || id > 3) return hd_fail(msg, cap, JDS_EINVAL, "bad DQT table header 0x%02X", s[q]);
        if (q + 65 > sl) return hd_fail(msg, cap, JDS_EINVAL, "truncated DQT");
        memcpy(qt[id], s + q + 1, 64);
        qdef[id] = true;
        q += 65;
      }
    } else if (m == 0xC4) {
      int64_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return hd_fail(msg, cap, JDS_EINVAL, "truncated DHT");
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return hd_fail(msg, cap, JDS_EINVAL, "bad DHT table header 0x%02X", s[q]);
        if (th > 1) return hd_fail(msg, cap, JDS_ENOTSUP, "Huffman table id %d (baseline has 0 and 1)", th);
        int nv = 0;
        for (int i = 0; i < 16; ++i) nv += s[q + 1 + i];
        if (nv > 256) return hd_fail(msg, cap, JDS_EINVAL, "DHT: BITS sum to %d symbols (more than 256)", nv);
        if (q + 17 + nv > sl) return hd_fail(msg, cap, JDS_EINVAL, "truncated DHT");
        jds_jfif_huff* h = &out->huff[2 * tc + th];
        if (out->n_scans && h->defined)
          return hd_fail(msg, cap, JDS_ENOTSUP, "Huffman table redefined between scans");
        memset(h, 0, sizeof *h);
        memcpy(h->bits, s + q + 1, 16);
        memcpy(h->vals, s + q + 17, (size_t)nv);
        h->n_vals = nv;
        HuffDecTab t;
        if (hd_build(h->bits, h->vals, &t) < 0)
          return hd_fail(msg, cap, JDS_EINVAL, "DHT %d/%d: BITS over-subscribe the code space", tc, th);
        h->defined = 1;
        q += 17 + nv;
      }
    } else if (m == 0xDA) {
      if (!sof) return hd_fail(msg, cap, JDS_EINVAL, "SOS before SOF0");
      if (sl < 1) return hd_fail(msg, cap, JDS_EINVAL, "SOS too short");
      const int ns = s[0];
      if (ns != 1) return hd_fail(msg, cap, JDS_ENOTSUP, "interleaved scan (Ns = %d): non-interleaved scans only", ns);
      if (sl != 6) return hd_fail(msg, cap, JDS_EINVAL, "SOS length does not match its component count");
      const int comp = s[1], td = s[2] >> 4, ta = s[2] & 15;
      if (comp < 1 || comp > 3) return hd_fail(msg, cap, JDS_EINVAL, "SOS names component %d", comp);
      if (seen[comp]) return hd_fail(msg, cap, JDS_ENOTSUP, "component %d has a second scan", comp);
      if (s[3] != 0 || s[4] != 63 || s[5] != 0)
        return hd_fail(msg, cap, JDS_ENOTSUP, "spectral selection / successive approximation (progressive scan parameters)");
      if (td > 1 || ta > 1) return hd_fail(msg, cap, JDS_EINVAL, "SOS table ids %d/%d", td, ta);
      if (!out->huff[td].defined || !out->huff[2 + ta].defined)
        return hd_fail(msg, cap, JDS_EINVAL, "SOS refers to a Huffman table the file has not defined");
      if (!qdef[tq]) return hd_fail(msg, cap, JDS_EINVAL, "quantisation table %d is not defined", tq);
      if (out->n_scans >= 3) return hd_fail(msg, cap, JDS_EINVAL, "more than three scans");
      seen[comp] = true;
      int64_t e = p + 2 + ln;
      // entropy-coded segment: up to the next marker (0xFF, then neither 0x00 nor a fill 0xFF);
      // with a restart interval in effect its RSTm markers belong to it, m = i & 7 for the i-th
      int64_t nm = 0;
      for (;;) {
        if (e + 1 >= len) return hd_fail(msg, cap, JDS_EINVAL, "truncated scan data: EOI missing");
        if (data[e] == 0xFF && data[e + 1] != 0x00) {
          const int r = data[e + 1] - 0xD0;
          if (r < 0 || r > 7) break;
          if (!ri)
            return hd_fail(msg, cap, JDS_EINVAL, "scan %d: restart marker RST%d without a restart interval (no DRI)",
                           out->n_scans, r);
          if (r != (int)(nm & 7))
            return hd_fail(msg, cap, JDS_EINVAL, "scan %d: restart marker RST%d where RST%d belongs (DRI %d)",
                           out->n_scans, r, (int)(nm & 7), ri);
          ++nm;
          e += 2;
          continue;
        }
        ++e;
      }
      if (ri) {
        int64_t ny = 0, nc = 0;
        const int brc = hd_block_counts(out->H, out->W, out->subsampling, &ny, &nc, msg, cap);
        if (brc) return brc;
        const int64_t nb = comp == 1 ? ny : nc, need = (nb + ri - 1) / ri - 1;
        if (nm != need)
          return hd_fail(msg, cap, JDS_EINVAL, "scan %d: %lld restart markers where DRI %d needs %lld", out->n_scans,
                         (long long)nm, ri, (long long)need);
        if (data[e + 1] == 0xFF)
          return hd_fail(msg, cap, JDS_ENOTSUP, "scan %d: fill bytes (FF FF) in scan data with a restart interval (DRI %d)",
                         out->n_scans, ri);
      }
      jds_jfif_scan* sc = &out->scan[out->n_scans++];
      sc->component = comp;
      sc->dc_table = td;
      sc->ac_table = ta;
      sc->restart_interval = ri;
      sc->offset = p + 2 + ln;
      sc->length = e - sc->offset;
      p = e;
      continue;
    }
    // APPn, COM and anything else with a length: skipped
    p += 2 + ln;
  }
  if (!sof) return hd_fail(msg, cap, JDS_EINVAL, "no SOF0 segment");
  if (!headers_only && out->n_scans != 3) return hd_fail(msg, cap, JDS_EINVAL, "%d scans (one per component expected)", out->n_scans);
  if (tq >= 0 && qdef[tq])
    for (int k = 0; k < 64; ++k) out->qtable[HD_ZZ[k]] = (double)qt[tq][k];
  else if (!headers_only)
    return hd_fail(msg, cap, JDS_EINVAL, "quantisation table %d is not defined", tq);
  int64_t ny = 0, nc = 0;
  const int rc = hd_block_counts(out->H, out->W, out->subsampling, &ny, &nc, msg, cap);
  if (rc) return rc;
  out->y_blocks = ny;
  out->c_blocks = nc;
  out->coeffs_needed = 64 * (ny + 2 * nc);
  return JDS_OK;
}

inline const char* hd_status_text(uint32_t st) {
  if (st & HD_BAD_HEADER) return "header mismatch or empty file";
  if (st & HD_RESTART) return "restart markers differ from what the geometry and the restart interval require";
  if (st & HD_BAD_CODE) return "invalid Huffman code in the scan data";
  if (st & HD_K63) return "coefficient index beyond 63 in the scan data";
  if (st & HD_OVERRUN) return "scan data overrun: the scan ends inside a symbol";
  if (st & HD_COUNT) return "block count mismatch: the scan does not hold exactly its blocks";
  if (st & HD_DC_RANGE) return "DC value outside int16";
  return "ok";
}

struct HdHostSink {
  int16_t* out;
  void operator()(int64_t blk, int k, int v) const { out[blk * 64 + HD_ZZ[k]] = (int16_t)v; }
};

// One scan on the host, a loop standing in for the lanes: subsequences of S
// bits, the propagation rule of the kernels (entry[i + 1] <- exit[i], changed
// entries decode again), block prefix, write pass, DC prefix sum.  out:
// nblocks x 64, zeroed here.  *rounds = decode rounds run.  Returns status bits.
template <class TC, class Sink>
inline uint32_t hd_host_sync(const uint8_t* d, int64_t n, const TC& tc, int64_t S, int64_t nblocks, Sink&& sink,
                             int32_t* rounds);

inline uint32_t hd_host_scan(const uint8_t* d, int64_t n, const HuffDecTab* dc, const HuffDecTab* ac, int64_t S,
                             int64_t nblocks, int16_t* out, int32_t* rounds) {
  memset(out, 0, sizeof(int16_t) * 64 * (size_t)nblocks);
  uint32_t st = hd_host_sync(d, n, HdPlain{dc, ac}, S, nblocks, HdHostSink{out}, rounds);
  int32_t acc = 0;
  for (int64_t b = 0; b < nblocks; ++b) {
    acc += out[64 * b];
    if (acc < -32768 || acc > 32767) st |= HD_DC_RANGE;
    out[64 * b] = (int16_t)acc;
  }
  return st;
}

// The rounds and the write pass of hd_host_scan for any table choice and sink
// (the caller zeroes the output and sums the DC differences).
template <class TC, class Sink>
inline uint32_t hd_host_sync(const uint8_t* d, int64_t n, const TC& tc, int64_t S, int64_t nblocks, Sink&& sink,
                             int32_t* rounds) {
  const HdMemSrc src{d, n};
  const int64_t nbits = 8 * n;
  const int64_t nsub = nbits ? (nbits + S - 1) / S : 1;
  std::vector<uint64_t> entry((size_t)nsub), exitv((size_t)nsub, HD_NONE);
  std::vector<uint32_t> nblk((size_t)nsub, 0u);
  std::vector<char> need((size_t)nsub, 1);
  for (int64_t i = 0; i < nsub; ++i) entry[(size_t)i] = i ? hd_guess(src, i * S) : 0;
  int32_t r = 0;
  for (;;) {
    bool any = false;
    for (int64_t i = 0; i < nsub; ++i)
      if (need[(size_t)i]) {
        exitv[(size_t)i] = hd_sync_lane(src, tc, entry[(size_t)i], (uint64_t)((i + 1) * S), nblk[(size_t)i]);
        any = true;
      }
    if (!any) break;
    ++r;
    if (r > nsub) break;  // cannot happen: entries 0..r are settled after round r
    for (int64_t i = nsub - 1; i >= 1; --i) {
      const uint64_t c = exitv[(size_t)i - 1];
      need[(size_t)i] = c != HD_NONE && c != entry[(size_t)i];
      if (need[(size_t)i]) entry[(size_t)i] = c;
    }
    need[0] = 0;
  }
  *rounds = r;
  uint32_t st = 0;
  int64_t b0 = 0;
  for (int64_t i = 0; i < nsub; ++i) {
    st |= hd_write_lane(src, tc, entry[(size_t)i], (uint64_t)((i + 1) * S), b0, nblocks, i == nsub - 1, sink);
    b0 += nblk[(size_t)i];
  }
  return st;
}

// DC differences -> values inside the lane of one restart interval, judged
// against int16 (the prediction starts from 0 at every interval).
struct HdRstHostSink {
  int16_t* out;
  int32_t acc = 0;
  bool bad = false;
  void operator()(int64_t blk, int k, int v) {
    if (k == 0) {
      acc += v;
      bad = bad || acc < -32768 || acc > 32767;
      v = acc;
    }
    out[blk * 64 + HD_ZZ[k]] = (int16_t)v;
  }
};

// One scan with restart interval ri on the host, a loop standing in for the
// lanes of k_dec_rst: the parser checked the markers' number and order, so
// interval i lies between markers i - 1 and i.  out: nblocks x 64, zeroed here.
inline uint32_t hd_host_scan_rst(const uint8_t* d, int64_t n, const HuffDecTab* dc, const HuffDecTab* ac, int64_t ri,
                                 int64_t nblocks, int16_t* out) {
  memset(out, 0, sizeof(int16_t) * 64 * (size_t)nblocks);
  uint32_t st = 0;
  int64_t a = 0, blk0 = 0;
  while (blk0 < nblocks) {
    int64_t e = a;
    while (e < n && !(d[e] == 0xFF && e + 1 < n && d[e + 1] >= 0xD0 && d[e + 1] <= 0xD7)) ++e;
    const int64_t nb = nblocks - blk0 < ri ? nblocks - blk0 : ri;
    HdRstHostSink sink{out};
    st |= hd_rst_lane(HdMemSrc{d + a, e - a}, HdPlain{dc, ac}, blk0, nb, sink);
    if (sink.bad) st |= HD_DC_RANGE;
    blk0 += nb;
    if (e >= n) break;
    a = e + 2;
  }
  if (blk0 < nblocks) st |= HD_RESTART;  // (the parser's marker count rules this out)
  return st;
}

// A whole parsed file on the host (jds_selftest_huffdec, tools/jfif_host_san.cpp).
// coeffs: info->coeffs_needed int16 in the reference layout.  rounds[3]: per
// component (Y, Cb, Cr).
inline uint32_t hd_host_decode(const uint8_t* data, const jds_jfif_info* info, int64_t S, int16_t* coeffs,
                               int32_t* rounds) {
  uint32_t st = 0;
  for (int i = 0; i < info->n_scans; ++i) {
    const jds_jfif_scan& sc = info->scan[i];
    HuffDecTab dc, ac;
    if (hd_build(info->huff[sc.dc_table].bits, info->huff[sc.dc_table].vals, &dc) < 0 ||
        hd_build(info->huff[2 + sc.ac_table].bits, info->huff[2 + sc.ac_table].vals, &ac) < 0)
      return HD_BAD_HEADER;
    const int c = sc.component - 1;
    const int64_t nb = c ? info->c_blocks : info->y_blocks;
    const int64_t off = c == 0 ? 0 : 64 * (info->y_blocks + (c - 1) * info->c_blocks);
    if (sc.restart_interval > 0) {  // every interval a stream of its own: no propagation rounds
      st |= hd_host_scan_rst(data + sc.offset, sc.length, &dc, &ac, sc.restart_interval, nb, coeffs + off);
      rounds[c] = 0;
    } else {
      st |= hd_host_scan(data + sc.offset, sc.length, &dc, &ac, S, nb, coeffs + off, rounds + c);
    }
  }
  return st;
}

// --------------------------------------------------- interleaved files --

// Parse a baseline JPEG of either scan form (include/jds.h: jds_jpeg_parse).
// Never reads outside [data, data + len).
inline int hd_jpeg_parse(const uint8_t* data, int64_t len, jds_jpeg_info* out, char* msg, size_t cap) {
  if (!data || !out || len < 0) return hd_fail(msg, cap, JDS_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) return hd_fail(msg, cap, JDS_EINVAL, "not a JPEG file: SOI missing");
  uint8_t qt[4][64];
  bool qdef[4] = {false, false, false, false};
  bool sof = false, seen[4] = {false, false, false, false};
  int ri = 0;
  int ncomp = 3, gray_id = 0;  // a one-component frame: its component id as written (the SOS must name it)
  int64_t p = 2;
  for (;;) {
    if (p + 2 > len) return hd_fail(msg, cap, JDS_EINVAL, "truncated file: EOI missing");
    if (data[p] != 0xFF) return hd_fail(msg, cap, JDS_EINVAL, "marker expected at byte %lld", (long long)p);
    const int m = data[p + 1];
    if (m == 0xFF) {  // fill byte
      ++p;
      continue;
    }
    if (m == 0xD9) break;  // EOI
    if (m >= 0xD0 && m <= 0xD7)
      return hd_fail(msg, cap, JDS_EINVAL, "restart marker RST%d outside scan data at byte %lld", m - 0xD0, (long long)p);
    if (m == 0xD8 || m == 0x01 || m == 0x00)
      return hd_fail(msg, cap, JDS_EINVAL, "unexpected marker 0x%02X at byte %lld", m, (long long)p);
    if (p + 4 > len) return hd_fail(msg, cap, JDS_EINVAL, "truncated segment header at byte %lld", (long long)p);
    const int64_t ln = ((int64_t)data[p + 2] << 8) | data[p + 3];
    if (ln < 2 || p + 2 + ln > len)
      return hd_fail(msg, cap, JDS_EINVAL, "segment 0x%02X at byte %lld: length %lld reaches past the end of the file", m,
                     (long long)p, (long long)ln);
    const uint8_t* s = data + p + 4;
    const int64_t sl = ln - 2;
    if (m == 0xC0) {
      if (sof) return hd_fail(msg, cap, JDS_EINVAL, "second SOF0");
      if (sl < 6) return hd_fail(msg, cap, JDS_EINVAL, "SOF0 too short");
      if (s[0] != 8) return hd_fail(msg, cap, JDS_ENOTSUP, "sample precision %d (12-bit and other depths are not supported)", s[0]);
      out->H = (s[1] << 8) | s[2];
      out->W = (s[3] << 8) | s[4];
      const int nf = s[5];
      if (nf != 1 && nf != 3) return hd_fail(msg, cap, JDS_ENOTSUP, "%d components (one or three are supported)", nf);
      if (sl != 6 + 3 * nf) return hd_fail(msg, cap, JDS_EINVAL, "SOF0 length does not match its component count");
      if (out->H < 1 || out->W < 1) return hd_fail(msg, cap, JDS_ENOTSUP, "frame size %lldx%lld (DNL is not supported)", (long long)out->H, (long long)out->W);
      if (nf == 1) {
        // grayscale: any component id; the sampling byte is checked and then ignored, since a
        // one-component scan is never interleaved and holds ceil(W/8) x ceil(H/8) blocks (T.81 A.2.2)
        const int h1 = s[7] >> 4, v1 = s[7] & 15;
        if (h1 < 1 || h1 > 4 || v1 < 1 || v1 > 4)
          return hd_fail(msg, cap, JDS_EINVAL, "sampling factors %dx%d (1..4 each)", h1, v1);
        if (s[8] > 3) return hd_fail(msg, cap, JDS_EINVAL, "quantisation table id %d", s[8]);
        ncomp = 1;
        gray_id = s[6];
        out->subsampling = JDS_SS_GRAY;
        out->tq[0] = s[8];
        out->hs[0] = out->vs[0] = 1;
        out->grid_cols[0] = out->mcu_cols = (out->W + 7) / 8;
        out->grid_rows[0] = out->mcu_rows = (out->H + 7) / 8;
        out->coeffs_needed = 64 * out->grid_cols[0] * out->grid_rows[0];
        out->single_table = 1;
        out->blocks_per_mcu = 1;
        sof = true;
        p += 2 + ln;
        continue;
      }
      for (int c = 0; c < 3; ++c)
        if (s[6 + 3 * c] != c + 1) return hd_fail(msg, cap, JDS_ENOTSUP, "component ids other than 1, 2, 3");
      const int ys = s[7];
      if (ys != 0x11 && ys != 0x21 && ys != 0x22)
        return hd_fail(msg, cap, JDS_ENOTSUP, "luma sampling %dx%d (1x1, 2x1 and 2x2 are supported)", ys >> 4, ys & 15);
      if (s[10] != 0x11 || s[13] != 0x11) return hd_fail(msg, cap, JDS_ENOTSUP, "subsampled or oversampled chroma factors");
      out->subsampling = ys == 0x11 ? JDS_SS_444 : (ys == 0x21 ? JDS_SS_422 : JDS_SS_420);
      const int hmax = ys >> 4, vmax = ys & 15;
      for (int c = 0; c < 3; ++c) {
        out->tq[c] = s[8 + 3 * c];
        if (out->tq[c] > 3) return hd_fail(msg, cap, JDS_EINVAL, "quantisation table id %d", out->tq[c]);
        out->hs[c] = c ? 1 : hmax;
        out->vs[c] = c ? 1 : vmax;
        const int64_t xc = (out->W * out->hs[c] + hmax - 1) / hmax, yc = (out->H * out->vs[c] + vmax - 1) / vmax;
        out->grid_cols[c] = (xc + 7) / 8;
        out->grid_rows[c] = (yc + 7) / 8;
        out->coeffs_needed += 64 * out->grid_cols[c] * out->grid_rows[c];
      }
      out->single_table = out->tq[0] == out->tq[1] && out->tq[0] == out->tq[2];
      out->blocks_per_mcu = hmax * vmax + 2;
      out->mcu_cols = (out->W + 8 * hmax - 1) / (8 * hmax);
      out->mcu_rows = (out->H + 8 * vmax - 1) / (8 * vmax);
      int64_t ny = 0, nc = 0;
      out->reference_grid = hd_block_counts(out->H, out->W, out->subsampling, &ny, &nc, nullptr, 0) == JDS_OK;
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8) {
      if (m == 0xCC || m >= 0xC9) return hd_fail(msg, cap, JDS_ENOTSUP, "arithmetic coding (marker 0x%02X) is not supported", m);
      return hd_fail(msg, cap, JDS_ENOTSUP, "%s (SOF%d) is not supported: baseline SOF0 only", m == 0xC2 ? "progressive JPEG" : "this frame type", m - 0xC0);
    } else if (m == 0xDD) {
      if (ln != 4) return hd_fail(msg, cap, JDS_EINVAL, "DRI segment of length %lld (4 expected)", (long long)ln);
      ri = (s[0] << 8) | s[1];
    } else if (m == 0xDB) {
      int64_t q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, id = s[q] & 15;
        if (pq == 1) return hd_fail(msg, cap, JDS_ENOTSUP, "16-bit DQT is not supported");
        if (pq != 0 || id > 3) return hd_fail(msg, cap, JDS_EINVAL, "bad DQT table header 0x%02X", s[q]);
        if (q + 65 > sl) return hd_fail(msg, cap, JDS_EINVAL, "truncated DQT");
        memcpy(qt[id], s + q + 1, 64);
        qdef[id] = true;
        q += 65;
      }
    } else if (m == 0xC4) {
      int64_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return hd_fail(msg, cap, JDS_EINVAL, "truncated DHT");
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return hd_fail(msg, cap, JDS_EINVAL, "bad DHT table header 0x%02X", s[q]);
        if (th > 1) return hd_fail(msg, cap, JDS_ENOTSUP, "Huffman table id %d (baseline has 0 and 1)", th);
        int nv = 0;
        for (int i = 0; i < 16; ++i) nv += s[q + 1 + i];
        if (nv > 256) return hd_fail(msg, cap, JDS_EINVAL, "DHT: BITS sum to %d symbols (more than 256)", nv);
        if (q + 17 + nv > sl) return hd_fail(msg, cap, JDS_EINVAL, "truncated DHT");
        jds_jfif_huff* h = &out->huff[2 * tc + th];
        if (out->n_scans && h->defined)
          return hd_fail(msg, cap, JDS_ENOTSUP, "Huffman table redefined between scans");
        memset(h, 0, sizeof *h);
        memcpy(h->bits, s + q + 1, 16);
        memcpy(h->vals, s + q + 17, (size_t)nv);
        h->n_vals = nv;
        HuffDecTab t;
        if (hd_build(h->bits, h->vals, &t) < 0)
          return hd_fail(msg, cap, JDS_EINVAL, "DHT %d/%d: BITS over-subscribe the code space", tc, th);
        h->defined = 1;
        q += 17 + nv;
      }
    } else if (m == 0xDA) {
      if (!sof) return hd_fail(msg, cap, JDS_EINVAL, "SOS before SOF0");
      if (sl < 1) return hd_fail(msg, cap, JDS_EINVAL, "SOS too short");
      const int ns = s[0];
      if (ncomp == 1 && ns != 1)
        return hd_fail(msg, cap, JDS_EINVAL, "scan of %d components in a grayscale (one-component) frame", ns);
      if (ncomp == 1 && out->n_scans)
        return hd_fail(msg, cap, JDS_ENOTSUP, "a second scan in a grayscale (one-component) file");
      if (ns == 2)
        return hd_fail(msg, cap, JDS_ENOTSUP, "interleaved scan of two components (Ns = 2): one scan of three or three of one only");
      if (ns != 1 && ns != 3) return hd_fail(msg, cap, JDS_EINVAL, "SOS with %d components", ns);
      if (sl != 4 + 2 * ns) return hd_fail(msg, cap, JDS_EINVAL, "SOS length does not match its component count");
      if (out->interleaved || (ns == 3 && out->n_scans))
        return hd_fail(msg, cap, JDS_ENOTSUP, "a mix of interleaved and non-interleaved scans");
      if (out->n_scans >= 3) return hd_fail(msg, cap, JDS_EINVAL, "more than three scans");
      jds_jpeg_scan* sc = &out->scan[out->n_scans];
      memset(sc, 0, sizeof *sc);
      for (int i = 0; i < ns; ++i) {
        int comp = s[1 + 2 * i];
        const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
        if (ncomp == 1) {
          if (comp != gray_id)
            return hd_fail(msg, cap, JDS_EINVAL, "SOS names component %d, the grayscale frame's component is %d", comp, gray_id);
          comp = 1;  // (the info counts components from 1; the file's own id stays in its header)
        }
        if (comp < 1 || comp > 3) return hd_fail(msg, cap, JDS_EINVAL, "SOS names component %d", comp);
        if (ns == 3 && comp != i + 1)
          return hd_fail(msg, cap, JDS_ENOTSUP, "interleaved scan whose components are not 1, 2, 3 in that order");
        if (seen[comp]) return hd_fail(msg, cap, JDS_ENOTSUP, "component %d has a second scan", comp);
        if (td > 1 || ta > 1) return hd_fail(msg, cap, JDS_EINVAL, "SOS table ids %d/%d", td, ta);
        if (!out->huff[td].defined || !out->huff[2 + ta].defined)
          return hd_fail(msg, cap, JDS_EINVAL, "SOS refers to a Huffman table the file has not defined");
        if (!qdef[out->tq[comp - 1]])
          return hd_fail(msg, cap, JDS_EINVAL, "quantisation table %d is not defined", out->tq[comp - 1]);
        seen[comp] = true;
        sc->component[i] = comp;
        sc->dc_table[i] = td;
        sc->ac_table[i] = ta;
      }
      const uint8_t* t = s + 1 + 2 * ns;
      if (t[0] != 0 || t[1] != 63 || t[2] != 0)
        return hd_fail(msg, cap, JDS_ENOTSUP, "spectral selection / successive approximation (progressive scan parameters)");
      int64_t e = p + 2 + ln;
      int64_t nm = 0;
      for (;;) {
        if (e + 1 >= len) return hd_fail(msg, cap, JDS_EINVAL, "truncated scan data: EOI missing");
        if (data[e] == 0xFF && data[e + 1] != 0x00) {
          const int r = data[e + 1] - 0xD0;
          if (r < 0 || r > 7) break;
          if (!ri)
            return hd_fail(msg, cap, JDS_EINVAL, "scan %d: restart marker RST%d without a restart interval (no DRI)",
                           out->n_scans, r);
          if (r != (int)(nm & 7))
            return hd_fail(msg, cap, JDS_EINVAL, "scan %d: restart marker RST%d where RST%d belongs (DRI %d)",
                           out->n_scans, r, (int)(nm & 7), ri);
          ++nm;
          e += 2;
          continue;
        }
        ++e;
      }
      if (ri) {
        const int c0 = sc->component[0] - 1;
        const int64_t nmcu = ns == 3 ? out->mcu_cols * out->mcu_rows : out->grid_cols[c0] * out->grid_rows[c0];
        const int64_t need = (nmcu + ri - 1) / ri - 1;
        if (nm != need)
          return hd_fail(msg, cap, JDS_EINVAL, "scan %d: %lld restart markers where DRI %d needs %lld", out->n_scans,
                         (long long)nm, ri, (long long)need);
        if (data[e + 1] == 0xFF)
          return hd_fail(msg, cap, JDS_ENOTSUP, "scan %d: fill bytes (FF FF) in scan data with a restart interval (DRI %d)",
                         out->n_scans, ri);
      }
      sc->n_components = ns;
      sc->restart_interval = ri;
      sc->offset = p + 2 + ln;
      sc->length = e - sc->offset;
      out->interleaved = ns == 3;
      ++out->n_scans;
      p = e;
      continue;
    }
    // APPn, COM and anything else with a length: skipped
    p += 2 + ln;
  }
  if (!sof) return hd_fail(msg, cap, JDS_EINVAL, "no SOF0 segment");
  if (out->n_scans != (out->interleaved || ncomp == 1 ? 1 : 3))
    return hd_fail(msg, cap, JDS_EINVAL, "%d scans (one interleaved scan or one per component expected)", out->n_scans);
  for (int c = 0; c < ncomp; ++c)
    for (int k = 0; k < 64; ++k) out->qtable[c][HD_ZZ[k]] = (double)qt[out->tq[c]][k];
  return JDS_OK;
}

// The MCU descriptor of a parsed file's interleaved scan.
inline HdMcu hd_jpeg_mcu(const jds_jpeg_info* info) {
  HdMcu m;
  memset(&m, 0, sizeof m);
  m.bpm = info->blocks_per_mcu;
  m.mcu_cols = (int32_t)info->mcu_cols;
  m.mcu_rows = (int32_t)info->mcu_rows;
  int slot = 0;
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    m.hs[c] = info->hs[c];
    m.vs[c] = info->vs[c];
    m.gw[c] = (int32_t)info->grid_cols[c];
    m.gh[c] = (int32_t)info->grid_rows[c];
    m.first[c] = slot;
    m.off[c] = off;
    off += 64 * info->grid_cols[c] * info->grid_rows[c];
    for (int j = 0; j < m.hs[c] * m.vs[c]; ++j, ++slot) {
      m.comp[slot] = (uint8_t)c;
      m.bx[slot] = (uint8_t)(j % m.hs[c]);
      m.by[slot] = (uint8_t)(j / m.hs[c]);
      m.dct[slot] = (uint8_t)info->scan[0].dc_table[c];
      m.act[slot] = (uint8_t)(2 + info->scan[0].ac_table[c]);
    }
  }
  return m;
}

// DC differences of an interleaved scan -> values (the host's k_dec_dc_mcu):
// per component a running sum over the staging array in scan order, padding
// blocks included, from 0 at blocks [b0, b1) (whole MCUs: a scan, or one
// restart interval); kept blocks get their value.
inline uint32_t hd_host_dc_mcu(const HdMcu* m, const int16_t* dcs, int64_t b0, int64_t b1, int16_t* coeffs) {
  int32_t acc[3] = {0, 0, 0};
  uint32_t st = 0;
  for (int64_t n = b0; n < b1; ++n) {
    int c;
    int16_t* dst = hd_il_place(m, coeffs, n, c);
    acc[c] += dcs[n];
    if (acc[c] < -32768 || acc[c] > 32767) st |= HD_DC_RANGE;
    if (dst) dst[0] = (int16_t)acc[c];
  }
  return st;
}

// A whole parsed file on the host (jds_selftest_jpegdec, tools/jfif_host_san.cpp):
// non-interleaved scans as hd_host_decode over the T.81 grids, an interleaved
// one with the lanes' rules: intervals of at most lane_max blocks one lane
// each, longer ones (and a scan without intervals) through the rounds.
// coeffs: info->coeffs_needed int16.  rounds[3]: per scan in file order.
inline uint32_t hd_jpeg_host_decode(const uint8_t* data, const jds_jpeg_info* info, int64_t S, int64_t lane_max,
                                    int16_t* coeffs, int32_t* rounds) {
  uint32_t st = 0;
  HuffDecTab tabs[4];
  for (int i = 0; i < 4; ++i) {
    memset(&tabs[i], 0, sizeof tabs[i]);
    if (info->huff[i].defined && hd_build(info->huff[i].bits, info->huff[i].vals, &tabs[i]) < 0) return HD_BAD_HEADER;
  }
  rounds[0] = rounds[1] = rounds[2] = 0;
  if (!info->interleaved) {
    for (int i = 0; i < info->n_scans; ++i) {
      const jds_jpeg_scan& sc = info->scan[i];
      const int c = sc.component[0] - 1;
      int64_t off = 0;
      for (int j = 0; j < c; ++j) off += 64 * info->grid_cols[j] * info->grid_rows[j];
      const int64_t nb = info->grid_cols[c] * info->grid_rows[c];
      const HuffDecTab *dc = &tabs[sc.dc_table[0]], *ac = &tabs[2 + sc.ac_table[0]];
      if (sc.restart_interval > 0)
        st |= hd_host_scan_rst(data + sc.offset, sc.length, dc, ac, sc.restart_interval, nb, coeffs + off);
      else
        st |= hd_host_scan(data + sc.offset, sc.length, dc, ac, S, nb, coeffs + off, rounds + i);
    }
    return st;
  }
  const HdMcu m = hd_jpeg_mcu(info);
  const HdIl tc{tabs, &m};
  const jds_jpeg_scan& sc = info->scan[0];
  const uint8_t* d = data + sc.offset;
  const int64_t n = sc.length, nblocks = (int64_t)m.bpm * m.mcu_cols * m.mcu_rows;
  memset(coeffs, 0, sizeof(int16_t) * (size_t)info->coeffs_needed);
  std::vector<int16_t> dcs((size_t)nblocks, 0);
  if (sc.restart_interval == 0) {
    st |= hd_host_sync(d, n, tc, S, nblocks, HdIlSink{&m, coeffs, dcs.data(), HD_ZZ, 0}, rounds);
    st |= hd_host_dc_mcu(&m, dcs.data(), 0, nblocks, coeffs);
    return st;
  }
  const int64_t rib = (int64_t)sc.restart_interval * m.bpm;
  int64_t a = 0, blk0 = 0;
  while (blk0 < nblocks) {
    int64_t e = a;
    while (e < n && !(d[e] == 0xFF && e + 1 < n && d[e + 1] >= 0xD0 && d[e + 1] <= 0xD7)) ++e;
    const int64_t nb = nblocks - blk0 < rib ? nblocks - blk0 : rib;
    if (rib <= lane_max) {
      HdIlRstSink sink{&m, coeffs, HD_ZZ, blk0};
      st |= hd_rst_lane(HdMemSrc{d + a, e - a}, tc, 0, nb, sink);
      if (sink.bad) st |= HD_DC_RANGE;
    } else {
      int32_t r = 0;
      st |= hd_host_sync(d + a, e - a, tc, S, nb, HdIlSink{&m, coeffs, dcs.data(), HD_ZZ, blk0}, &r);
      st |= hd_host_dc_mcu(&m, dcs.data(), blk0, blk0 + nb, coeffs);
      rounds[0] = r > rounds[0] ? r : rounds[0];
    }
    blk0 += nb;
    if (e >= n) break;
    a = e + 2;
  }
  if (blk0 < nblocks) st |= HD_RESTART;
  return st;
}

}  // namespace jds
