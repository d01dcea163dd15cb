// jds_pjpeg_dec.hpp — the decode core of progressive files (T.81 Annex G;
// DESIGN.md "Progressive files").  Compiles for host and device: the lane of
// k_pjpeg_chains (jds_pjpeg_dec.hip), the host model behind
// jds_selftest_pjpegdec and the stand-alone sanitizer program
// (tools/pjpeg_san.cpp) run this same code.  No HIP types here.
//
// The unit of work is a chain: the scans of one file that touch the same
// coefficients, in file order -- all DC scans (index 0 of every block), or the
// AC scans of one component (indices 1..63 of its plane).  One lane walks a
// chain sequentially.  Chains write disjoint int16 entries, so every access to
// the coefficients is a plain 16-bit load or store of the lane's own entries:
// a block's DC and its AC 1 share a dword and belong to different lanes.
#pragma once
#include "jds_huffdec.hpp"

namespace jds {

// One scan of a chain (host-built, jds_pjpeg_parse.hpp).
struct PjScan {
  long long data_off;  // the entropy-coded segment, from the source's byte 0
  long long nbytes;
  int32_t ns;       // components: 1 or 3
  int32_t comp[3];  // 0-based, in scan order
  int32_t tab[3];   // per scan component: index into the table array (DC scan: its DC table; AC: its AC table); -1: none
  int32_t ss, se, ah, al;
  int32_t ri;  // restart interval in MCUs of this scan; 0: none
  int32_t pad_;
};

// A chain of one file: scans [scan0, scan0 + nscans) of the scan array.
struct PjChain {
  int32_t file;  // MCU record and status word
  int32_t scan0, nscans;
  int32_t pad_;
};

JDS_HDI int pj_zz(int k) {
  constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

// Bit reader over bytes [pos, end) of a source: 0xFF 0x00 is the data byte
// 0xFF; any other marker, or the end, stops the data, and what is read beyond
// are zero bits that count as `fake`.  The real bits are always the top ones
// of acc, so the reader has run dry exactly when cnt < fake.
template <class Src>
struct PjBits {
  const Src& src;
  int64_t pos, end;
  uint64_t acc = 0;  // the next bits, left-aligned
  int cnt = 0;       // valid bits in acc, fake ones included
  int fake = 0;
  JDS_HDI PjBits(const Src& s, int64_t p, int64_t e) : src(s), pos(p), end(e) {}
  JDS_HDI void fill() {
    while (cnt <= 56) {
      uint32_t b = 0;
      bool real = false;
      if (!fake && pos < end) {
        b = src.byte(pos);
        if (b != 0xFFu) {
          real = true;
          ++pos;
        } else if (pos + 1 < end && src.byte(pos + 1) == 0x00u) {
          real = true;
          pos += 2;
        }
      }
      if (!real) {
        b = 0;
        fake += 8;
      }
      acc |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  JDS_HDI uint32_t peek16() {
    if (cnt < 16) fill();
    return (uint32_t)(acc >> 48);
  }
  JDS_HDI void skip(int n) {
    acc <<= n;
    cnt -= n;
  }
  JDS_HDI uint32_t get(int n) {  // 0 <= n <= 16
    if (n == 0) return 0;
    if (cnt < n) fill();
    const uint32_t v = (uint32_t)(acc >> (64 - n));
    skip(n);
    return v;
  }
  JDS_HDI bool dry() const { return cnt < fake; }
  // At a restart boundary or the scan's end: fewer than 8 real bits are left
  // (the pad bits of the last data byte).
  JDS_HDI bool at_byte_end() const { return cnt - fake >= 0 && cnt - fake < 8; }
  // The marker RSTm at pos; the reader starts over behind it.
  JDS_HDI bool restart(int m) {
    if (!at_byte_end() || pos + 1 >= end || src.byte(pos) != 0xFFu || src.byte(pos + 1) != (uint32_t)(0xD0 + m)) return false;
    pos += 2;
    acc = 0;
    cnt = fake = 0;
    return true;
  }
};

// One Huffman symbol; -1: a code not in the table.
template <class Src>
JDS_HDI int pj_sym(PjBits<Src>& br, const HuffDecTab* t) {
  const uint32_t v = br.peek16();
  const uint32_t e = t->lut[v >> 8];
  if (e) {
    br.skip((int)(e >> 8));
    return (int)(e & 255u);
  }
  for (int l = 9; l <= 16; ++l)
    if (v < t->limit[l - 9]) {
      br.skip(l);
      return t->vals[(uint32_t)(t->offs[l - 9] + (int32_t)(v >> (16 - l))) & 255u];
    }
  return -1;
}

// T.81 F.2.2.1 EXTEND of an s-bit magnitude (1 <= s <= 15).
JDS_HDI int32_t pj_extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int32_t)v - (int32_t)(1u << s) + 1 : (int32_t)v; }

// Plain int16 entries of a coefficient buffer.
struct PjCoefSink {
  int16_t* coeffs;
  JDS_HDI int32_t ld(const int16_t* p) const { return *p; }
  JDS_HDI void st(int16_t* p, int32_t v) const { *p = (int16_t)(uint16_t)(uint32_t)v; }  // the defined truncation
};

// A correction bit for a coefficient with history (G.1.2.3).
template <class Src, class Sink>
JDS_HDI void pj_correct(PjBits<Src>& br, const Sink& sink, int16_t* p, int32_t c, int32_t p1) {
  if (br.get(1)) sink.st(p, c >= 0 ? c + p1 : c - p1);
}

// One scan of a chain over the file's blocks.  tabs[j]: the table of scan
// component j (null where the scan reads none).  m: the file's MCU record,
// whose off[] count from sink.coeffs.  Returns the JDS_DEC_* bits met; the walk
// ends at the first.  Loops are bounded by the blocks and the band; the reader
// never leaves [data_off, data_off + nbytes); stores go to kept blocks of the
// file's own grids only.
template <class Src, class Sink>
JDS_HDI uint32_t hd_pjpeg_scan(const Src& src, const HuffDecTab* const* tabs, const PjScan& sc, const HdMcu& m,
                               const Sink& sink) {
  PjBits<Src> br(src, sc.data_off, sc.data_off + sc.nbytes);
  const bool il = sc.ns > 1, dc = sc.ss == 0;
  const int c0 = sc.comp[0];
  const int64_t nmcu = il ? (int64_t)m.mcu_cols * m.mcu_rows : (int64_t)m.gw[c0] * m.gh[c0];
  const int bpm = il ? m.bpm : 1;
  const int32_t p1 = (int32_t)(1u << sc.al);
  int32_t pred[3] = {0, 0, 0};
  int64_t eobrun = 0;  // blocks still covered by an end-of-band run, this one excluded
  int64_t left = sc.ri ? sc.ri : nmcu;  // MCUs up to the next restart marker
  int rst = 0;
  for (int64_t mcu = 0; mcu < nmcu; ++mcu) {
    if (left == 0) {
      if (!br.restart(rst)) return HD_RESTART;
      rst = (rst + 1) & 7;
      left = sc.ri;
      pred[0] = pred[1] = pred[2] = 0;
      eobrun = 0;  // (a run never crosses the boundary: checked where it is read)
    }
    for (int slot = 0; slot < bpm; ++slot) {
      int c = c0, j = 0;
      int16_t* blk;
      if (il) {
        blk = hd_il_place(&m, sink.coeffs, mcu * bpm + slot, c);
        j = c;  // (an interleaved scan names components 0, 1, 2 in order)
      } else {
        blk = sink.coeffs + m.off[c0] + 64 * mcu;
      }
      if (dc) {
        if (sc.ah == 0) {
          const int s = pj_sym(br, tabs[j]);
          if (s < 0 || s > 15) return HD_BAD_CODE;
          const int32_t d = s ? pj_extend(br.get(s), s) : 0;
          pred[j] += d;  // |pred| <= 32767 before, |d| <= 32767: no overflow
          if (pred[j] < -32768 || pred[j] > 32767) return HD_DC_RANGE;
          if (blk) sink.st(blk, (int32_t)((uint32_t)pred[j] << sc.al));
        } else {
          const uint32_t b = br.get(1);  // (a padding block's bit is consumed and dropped)
          if (blk && b) sink.st(blk, sink.ld(blk) | p1);
        }
      } else if (sc.ah == 0) {  // AC first pass (G.1.2.2)
        if (eobrun > 0) {
          --eobrun;
        } else {
          for (int k = sc.ss; k <= sc.se;) {
            const int rs = pj_sym(br, tabs[0]);
            if (rs < 0) return HD_BAD_CODE;
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
              if (r < 15) {  // EOBr: this block and run - 1 more end here
                const int64_t run = ((int64_t)1 << r) + (int64_t)br.get(r);
                if (run > left) return HD_COUNT;
                eobrun = run - 1;
                break;
              }
              k += 16;
              if (k > sc.se) return HD_K63;
            } else {
              k += r;
              if (k > sc.se) return HD_K63;
              const int32_t v = pj_extend(br.get(s), s);
              sink.st(blk + pj_zz(k), (int32_t)((uint32_t)v << sc.al));
              ++k;
            }
          }
        }
      } else {  // AC refinement (G.1.2.3)
        int k = sc.ss;
        if (eobrun == 0) {
          while (k <= sc.se) {
            const int rs = pj_sym(br, tabs[0]);
            if (rs < 0) return HD_BAD_CODE;
            int r = rs >> 4;
            const int s = rs & 15;
            int32_t nv = 0;
            if (s) {
              if (s != 1) return HD_BAD_CODE;
              nv = br.get(1) ? p1 : -p1;
            } else if (r < 15) {
              const int64_t run = ((int64_t)1 << r) + (int64_t)br.get(r);
              if (run > left) return HD_COUNT;
              eobrun = run;  // this block included: its corrections follow below
              break;
            }
            // pass r coefficients without history (ZRL: 16), correcting the ones with
            bool placed = false;
            while (k <= sc.se) {
              int16_t* p = blk + pj_zz(k);
              const int32_t cv = sink.ld(p);
              if (cv != 0) {
                pj_correct(br, sink, p, cv, p1);
              } else if (--r < 0) {
                if (s) sink.st(p, nv);
                placed = true;
                ++k;
                break;
              }
              ++k;
            }
            if (!placed) return HD_K63;  // the run or the new coefficient has no place up to Se
          }
        }
        if (eobrun > 0) {
          for (; k <= sc.se; ++k) {
            int16_t* p = blk + pj_zz(k);
            const int32_t cv = sink.ld(p);
            if (cv != 0) pj_correct(br, sink, p, cv, p1);
          }
          --eobrun;
        }
      }
      if (br.dry()) return HD_OVERRUN;
    }
    --left;
  }
  // the scan holds exactly its blocks: what is left are the last byte's pad bits
  if (br.pos < br.end || !br.at_byte_end()) return HD_COUNT;
  return 0;
}

// A chain: its scans in file order, ended by the first defect.  tab_base: the
// table array the scans' tab[] index.
template <class Src, class Sink>
JDS_HDI uint32_t hd_pjpeg_chain(const Src& src, const HuffDecTab* tab_base, const PjScan* scans, int nscans,
                                const HdMcu& m, const Sink& sink) {
  for (int i = 0; i < nscans; ++i) {
    const HuffDecTab* t[3];
    for (int j = 0; j < 3; ++j) t[j] = scans[i].tab[j] >= 0 ? tab_base + scans[i].tab[j] : nullptr;
    const uint32_t st = hd_pjpeg_scan(src, t, scans[i], m, sink);
    if (st) return st;
  }
  return 0;
}

}  // namespace jds
