// jds_huffdec.hpp — the Huffman decode core of the self-synchronising entropy
// decoder (jds_entropy_dec.hip; DESIGN.md "Entropy decode").  Compiles for
// host and device: the GPU lanes, the host model behind jds_selftest_huffdec
// (jds_jpeg_parse.hpp, with the header parser) and the stand-alone sanitizer
// program (tools/jfif_host_san.cpp) run this same code.  No HIP types here.  Scans
// with restart intervals (DRI) decode one interval per lane (hd_rst_lane).
//
// Stream positions are bit positions in the STUFFED scan bytes: the reader
// skips the 0x00 after every 0xFF itself, so a position never points into a
// stuffed byte.  A decoder state is (p, k, slot): p the position of the next
// symbol, k the zigzag index it belongs to (0: a DC symbol is expected), slot
// the block's index within its MCU (always 0 in a non-interleaved scan, whose
// MCU is one block), packed as p << 16 | slot << 8 | k.
#pragma once
#include <stdint.h>
#include <string.h>

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

// row-major index of the k-th zigzag coefficient (the host model's sinks, the parser's tables)
static const uint8_t HD_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                  58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

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
// index the whole table array.  Plans leave file at 0; so does a single-file
// call, the batch of one.
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

}  // namespace jds
