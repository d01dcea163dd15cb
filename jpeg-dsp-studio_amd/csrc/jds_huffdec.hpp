// jds_huffdec.hpp — baseline JFIF parsing and the Huffman decode core of the
// self-synchronising entropy decoder (jds_entropy_dec.hip; DESIGN.md "Entropy
// decode").  Compiles for host and device: the GPU lanes, the host model behind
// jds_selftest_huffdec and the stand-alone sanitizer program
// (tools/jfif_host_san.cpp) run this same code.  No HIP types here.  Scans
// with restart intervals (DRI) decode one interval per lane (hd_rst_lane).
//
// Stream positions are bit positions in the STUFFED scan bytes: the reader
// skips the 0x00 after every 0xFF itself, so a position never points into a
// stuffed byte.  A decoder state is (p, k): p the position of the next symbol,
// k the zigzag index it belongs to (0: a DC symbol is expected), packed as
// p << 8 | k.
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

JDS_HDI uint64_t hd_pack(uint64_t p, int k) { return (p << 8) | (uint64_t)(uint32_t)k; }

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

// Decode from (p, k) while p < pend and blk < blk_end: one symbol per
// iteration, DC and AC through the same body.  sink(blk, k, value) receives
// every coefficient (the DC entry is the difference).  Returns the defect bits
// met (the decode stops there).  Reads are bounded by the source's scan.
template <class Src, class Sink>
JDS_HDI uint32_t hd_run(const Src& src, const HuffDecTab* dc, const HuffDecTab* ac, uint64_t& p, int& k,
                        uint64_t pend, int64_t& blk, int64_t blk_end, Sink&& sink) {
  const uint64_t nbits = (uint64_t)src.n * 8u;
  while (p < pend && p < nbits && blk < blk_end) {
    uint64_t w;
    uint32_t ffm;
    hd_window(src, (int64_t)(p >> 3), w, ffm);
    const uint32_t off = (uint32_t)(p & 7u);
    const uint32_t x = (uint32_t)((w << (24u + off)) >> 32);  // the next 32 bits
    const uint32_t v = x >> 16;
    const bool isdc = k == 0;
    const HuffDecTab* t = isdc ? dc : ac;
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
      }
    } else {
      k += (int)run;
      if (k > 63) return HD_K63;
      sink(blk, k, val);
      if (++k == 64) {
        k = 0;
        ++blk;
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
template <class Src>
JDS_HDI uint64_t hd_sync_lane(const Src& src, const HuffDecTab* dc, const HuffDecTab* ac, uint64_t entry,
                              uint64_t pend, uint32_t& nblk) {
  uint64_t p = entry >> 8;
  int k = (int)(entry & 255u);
  int64_t blk = 0;
  const uint32_t fl = hd_run(src, dc, ac, p, k, pend, blk, (int64_t)1 << 62, HdNullSink());
  nblk = (uint32_t)blk;
  return (fl & (HD_BAD_CODE | HD_K63)) ? HD_NONE : hd_pack(p, k);
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
// (0, 0) over the interval's stuffed bytes, nblk blocks to the sink from block
// blk0 on (the sink sums the DC differences from 0 itself).  Judged alone: the
// interval must hold exactly its blocks and end in its pad bits.  The GPU lane
// (k_dec_rst) and the host model run this.
template <class Src, class Sink>
JDS_HDI uint32_t hd_rst_lane(const Src& src, const HuffDecTab* dc, const HuffDecTab* ac, int64_t blk0, int64_t nblk,
                             Sink&& sink) {
  uint64_t p = 0;
  int k = 0;
  int64_t blk = blk0;
  const uint32_t fl = hd_run(src, dc, ac, p, k, (uint64_t)src.n * 8u, blk, blk0 + nblk, sink);
  if (fl) return fl;
  if (blk != blk0 + nblk) return HD_COUNT;
  return hd_tail_ok(src, p) ? 0u : (uint32_t)HD_COUNT;
}

// Write pass of one subsequence, from its settled entry state and first block
// index; judges the scan: defects of the decode, data after the last block,
// or too few blocks (reported by the scan's last subsequence).
template <class Src, class Sink>
JDS_HDI uint32_t hd_write_lane(const Src& src, const HuffDecTab* dc, const HuffDecTab* ac, uint64_t entry,
                               uint64_t pend, int64_t blk0, int64_t nblocks, bool last, Sink&& sink) {
  if (entry == HD_NONE) return last ? HD_COUNT : 0;
  if (blk0 >= nblocks) return 0;
  uint64_t p = entry >> 8;
  int k = (int)(entry & 255u);
  int64_t blk = blk0;
  uint32_t fl = hd_run(src, dc, ac, p, k, pend, blk, nblocks, sink);
  if (fl) return fl;
  if (blk == nblocks) {
    // the scan is complete: what follows must be the final data byte's pad bits
    if (!hd_tail_ok(src, p)) fl |= HD_COUNT;
  } else if (last) {
    fl |= HD_COUNT;
  }
  return fl;
}

// One scan of one frame (host-built, jds_abi.hip).
struct DecScan {
  long long data_off;  // the scan's stuffed bytes, from the files base
  long long nbytes;
  long long coef_off;  // the scan's first coefficient, from the coeffs base
  int nblocks;
  int frame;
  int dc_tab, ac_tab;  // indices into the table array
  int grp0, ngrp;      // its workgroups
  int nsub;            // its subsequences
  int pad_;
};

// One restart interval of one frame (k_dec_rst): built on the host for a
// parsed file, on the device (k_rst_scan) for a plan's batch.  nblk == 0: not
// decoded (its frame is skipped).
struct RstIv {
  long long data_off;  // the interval's stuffed bytes, from the files base
  long long coef_off;  // its first block's first coefficient, from the coeffs base
  int nbytes;
  int nblk;
  int frame;
  int tabs;  // dc table index | ac table index << 8 (into the table array)
};

// What a plan knows about its restart files before it sees them.
struct RstGeo {
  int ri;           // the interval, in blocks
  int nblk[3];      // blocks of the Y, Cb, Cr scans
  int first[4];     // first interval of each scan within the frame; first[3]: intervals per frame
  long long off[3];  // the scans' first coefficient within the frame
  long long cpf;     // coefficients per frame
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
inline uint32_t hd_host_scan(const uint8_t* d, int64_t n, const HuffDecTab* dc, const HuffDecTab* ac, int64_t S,
                             int64_t nblocks, int16_t* out, int32_t* rounds) {
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
        exitv[(size_t)i] = hd_sync_lane(src, dc, ac, entry[(size_t)i], (uint64_t)((i + 1) * S), nblk[(size_t)i]);
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
  memset(out, 0, sizeof(int16_t) * 64 * (size_t)nblocks);
  uint32_t st = 0;
  int64_t b0 = 0;
  for (int64_t i = 0; i < nsub; ++i) {
    st |= hd_write_lane(src, dc, ac, entry[(size_t)i], (uint64_t)((i + 1) * S), b0, nblocks, i == nsub - 1,
                        HdHostSink{out});
    b0 += nblk[(size_t)i];
  }
  int32_t acc = 0;
  for (int64_t b = 0; b < nblocks; ++b) {
    acc += out[64 * b];
    if (acc < -32768 || acc > 32767) st |= HD_DC_RANGE;
    out[64 * b] = (int16_t)acc;
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
    st |= hd_rst_lane(HdMemSrc{d + a, e - a}, dc, ac, blk0, nb, sink);
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

}  // namespace jds
