// jds_jpeg_parse.hpp — the baseline JPEG header parser and the host model of
// the entropy decode (DESIGN.md "Entropy decode", "Interleaved scans").
//
// Host only and HIP-free: the C-ABI (jds_abi_jpeg.hip), the work-list builder
// (jds_dec_jobs.hpp) and the stand-alone sanitizer programs (tools/*_san.cpp)
// compile it; the lane routines it drives are the kernels' (jds_huffdec.hpp).
//
// One marker walk (hd_walk) reads every file into a jds_jpeg_info.  A file of
// the profile this library writes is such an info under restrictions (three
// Ns = 1 scans, one quantisation table, the reference's block grids, no
// grayscale): HD_OWN applies them, and jfif_info_of turns the result into the
// older public struct.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jds_huffdec.hpp"

namespace jds {

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

// HD_ANY: a baseline JPEG of either scan form (include/jds.h: jds_jpeg_parse).
// HD_OWN: the profile this library writes (jds_jfif_parse), a restriction of
// the former; the two differ only where the walk says `own` (DESIGN.md "One
// parser, two profiles").
enum HdProfile { HD_ANY, HD_OWN };

// ---- the pieces of a marker walk, shared by the baseline walk (hd_walk) and
// the progressive one (hd_pjpeg_parse, jds_pjpeg_parse.hpp): each check and its
// message is written once.  None reads outside [data, data + len).
struct HdWalk {
  const uint8_t* data;
  int64_t len;
  char* msg;
  size_t cap;
  int64_t p = 2;  // where the next segment is looked for (an SOS moves it behind its scan data)
  int m = 0;  // the segment at hand: marker FF m, payload s[0 .. sl)
  int64_t sl = 0;
  const uint8_t* s = nullptr;
  uint8_t qt[4][64];  // DQT: the tables as written (zig-zag order), and which are defined
  bool qdef[4] = {false, false, false, false};
  int ri = 0;  // the restart interval in effect (DRI), 0: none
  bool sof = false;
  int ncomp = 3, gray_id = 0;  // a one-component frame: its component id as written (the SOS must name it)
  template <class... A>
  int fail(int code, const char* fmt, A... a) const {
    return hd_fail(msg, cap, code, fmt, a...);
  }
};

// The next segment a walk has to look at: a frame header (SOFn), DHT, SOS, or
// EOI (m = 0xD9, no payload).  Fill bytes are passed over, DRI and DQT taken in,
// APPn, COM and anything else with a length skipped.
inline int hd_next(HdWalk& w) {
  const uint8_t* data = w.data;
  for (int64_t p = w.p;;) {
    if (p + 2 > w.len) return w.fail(JDS_EINVAL, "truncated file: EOI missing");
    if (data[p] != 0xFF) return w.fail(JDS_EINVAL, "marker expected at byte %lld", (long long)p);
    const int m = w.m = data[p + 1];
    if (m == 0xFF) {  // fill byte
      ++p;
      continue;
    }
    if (m == 0xD9) return JDS_OK;
    if (m >= 0xD0 && m <= 0xD7)
      return w.fail(JDS_EINVAL, "restart marker RST%d outside scan data at byte %lld", m - 0xD0, (long long)p);
    if (m == 0xD8 || m == 0x01 || m == 0x00)
      return w.fail(JDS_EINVAL, "unexpected marker 0x%02X at byte %lld", m, (long long)p);
    if (p + 4 > w.len) return w.fail(JDS_EINVAL, "truncated segment header at byte %lld", (long long)p);
    const int64_t ln = ((int64_t)data[p + 2] << 8) | data[p + 3];
    if (ln < 2 || p + 2 + ln > w.len)
      return w.fail(JDS_EINVAL, "segment 0x%02X at byte %lld: length %lld reaches past the end of the file", m,
                     (long long)p, (long long)ln);
    const uint8_t* s = w.s = data + p + 4;
    const int64_t sl = w.sl = ln - 2;
    w.p = p = p + 2 + ln;
    if ((m >= 0xC0 && m <= 0xCF && m != 0xC8) || m == 0xDA) return JDS_OK;
    if (m == 0xDD) {
      if (ln != 4) return w.fail(JDS_EINVAL, "DRI segment of length %lld (4 expected)", (long long)ln);
      w.ri = (s[0] << 8) | s[1];
    }
    for (int64_t q = 0; m == 0xDB && q < sl; q += 65) {
      const int pq = s[q] >> 4, id = s[q] & 15;
      if (pq == 1) return w.fail(JDS_ENOTSUP, "16-bit DQT is not supported");
      if (pq != 0 || id > 3) return w.fail(JDS_EINVAL, "bad DQT table header 0x%02X", s[q]);
      if (q + 65 > sl) return w.fail(JDS_EINVAL, "truncated DQT");
      memcpy(w.qt[id], s + q + 1, 64);
      w.qdef[id] = true;
    }
  }
}

// The frame header at hand, `name` ("SOF0", "SOF2") in its messages, into out:
// size, subsampling, tq, hs, vs, the grids, coeffs_needed, single_table,
// blocks_per_mcu, the MCU grid and reference_grid; w.ncomp and w.gray_id.
inline int hd_frame(HdWalk& w, const char* name, bool own, jds_jpeg_info* out) {
  const uint8_t* s = w.s;
  if (w.sof) return w.fail(JDS_EINVAL, "second %s", name);
  if (w.sl < 6) return w.fail(JDS_EINVAL, "%s too short", name);
  if (s[0] != 8) return w.fail(JDS_ENOTSUP, "sample precision %d (12-bit and other depths are not supported)", s[0]);
  out->H = (s[1] << 8) | s[2];
  out->W = (s[3] << 8) | s[4];
  const int nf = s[5];
  if (own && nf == 1) return w.fail(JDS_ENOTSUP, "grayscale files (one component) are not supported");
  if (nf != 3 && (own || nf != 1))
    return w.fail(JDS_ENOTSUP, "%d components (%s are supported)", nf, own ? "three" : "one or three");
  if (w.sl != 6 + 3 * nf) return w.fail(JDS_EINVAL, "%s length does not match its component count", name);
  if (out->H < 1 || out->W < 1)
    return w.fail(JDS_ENOTSUP, "frame size %lldx%lld (DNL is not supported)", (long long)out->H, (long long)out->W);
  if (nf == 1) {
    // grayscale: any component id; the sampling byte is checked and then ignored, since a
    // one-component scan is never interleaved and holds ceil(W/8) x ceil(H/8) blocks (T.81 A.2.2)
    const int h1 = s[7] >> 4, v1 = s[7] & 15;
    if (h1 < 1 || h1 > 4 || v1 < 1 || v1 > 4) return w.fail(JDS_EINVAL, "sampling factors %dx%d (1..4 each)", h1, v1);
    w.gray_id = s[6];
    out->subsampling = JDS_SS_GRAY;
  } else {
    for (int c = 0; c < 3; ++c)
      if (s[6 + 3 * c] != c + 1) return w.fail(JDS_ENOTSUP, "component ids other than 1, 2, 3");
    const int ys = s[7];
    if (ys != 0x11 && ys != 0x21 && ys != 0x22)
      return w.fail(JDS_ENOTSUP, "luma sampling %dx%d (1x1, 2x1 and 2x2 are supported)", ys >> 4, ys & 15);
    if (s[10] != 0x11 || s[13] != 0x11) return w.fail(JDS_ENOTSUP, "subsampled or oversampled chroma factors");
    out->subsampling = ys == 0x11 ? JDS_SS_444 : (ys == 0x21 ? JDS_SS_422 : JDS_SS_420);
    if (own && (s[8] != s[11] || s[8] != s[14]))
      return w.fail(JDS_ENOTSUP, "two quantisation tables in use (one is supported)");
  }
  w.ncomp = nf;
  const int hmax = nf == 1 ? 1 : s[7] >> 4, vmax = nf == 1 ? 1 : s[7] & 15;
  for (int c = 0; c < nf; ++c) {
    out->tq[c] = s[8 + 3 * c];
    if (out->tq[c] > 3) return w.fail(JDS_EINVAL, "quantisation table id %d", out->tq[c]);
    out->hs[c] = c ? 1 : hmax;
    out->vs[c] = c ? 1 : vmax;
    const int64_t xc = (out->W * out->hs[c] + hmax - 1) / hmax, yc = (out->H * out->vs[c] + vmax - 1) / vmax;
    out->grid_cols[c] = (xc + 7) / 8;
    out->grid_rows[c] = (yc + 7) / 8;
    out->coeffs_needed += 64 * out->grid_cols[c] * out->grid_rows[c];
  }
  out->single_table = nf == 1 || (out->tq[0] == out->tq[1] && out->tq[0] == out->tq[2]);
  out->blocks_per_mcu = nf == 1 ? 1 : hmax * vmax + 2;
  out->mcu_cols = (out->W + 8 * hmax - 1) / (8 * hmax);
  out->mcu_rows = (out->H + 8 * vmax - 1) / (8 * vmax);
  int64_t ny = 0, nc = 0;
  out->reference_grid = nf == 3 && hd_block_counts(out->H, out->W, out->subsampling, &ny, &nc, nullptr, 0) == JDS_OK;
  w.sof = true;
  return JDS_OK;
}

// A frame header other than the walk's own; only: the tail of the message.
inline int hd_refuse_sof(const HdWalk& w, const char* only) {
  if (w.m == 0xCC || w.m >= 0xC9) return w.fail(JDS_ENOTSUP, "arithmetic coding (marker 0x%02X) is not supported", w.m);
  return w.fail(JDS_ENOTSUP, "%s (SOF%d) is not supported: %s", w.m == 0xC2 ? "progressive JPEG" : "this frame type",
                 w.m - 0xC0, only);
}

// The table at byte q of the DHT at hand: Tc/Th (th_max: the highest id the walk
// takes, 3 by T.81), BITS, its nv values within the segment, and its codes.
// fixed (nullable): the file's tables [2 * Tc + Th] once a scan has used them.
inline int hd_dht_table(const HdWalk& w, int64_t q, int th_max, const jds_jfif_huff* fixed, int* tc, int* th, int* nv) {
  const uint8_t* s = w.s + q;
  if (q + 17 > w.sl) return w.fail(JDS_EINVAL, "truncated DHT");
  *tc = s[0] >> 4;
  *th = s[0] & 15;
  if (*tc > 1 || *th > 3) return w.fail(JDS_EINVAL, "bad DHT table header 0x%02X", s[0]);
  if (*th > th_max) return w.fail(JDS_ENOTSUP, "Huffman table id %d (baseline has 0 and 1)", *th);
  *nv = 0;
  for (int i = 0; i < 16; ++i) *nv += s[1 + i];
  if (*nv > 256) return w.fail(JDS_EINVAL, "DHT: BITS sum to %d symbols (more than 256)", *nv);
  if (q + 17 + *nv > w.sl) return w.fail(JDS_EINVAL, "truncated DHT");
  if (fixed && fixed[2 * *tc + *th].defined) return w.fail(JDS_ENOTSUP, "Huffman table redefined between scans");
  uint8_t vals[256];
  memset(vals, 0, sizeof vals);
  memcpy(vals, s + 17, (size_t)*nv);
  HuffDecTab t;
  if (hd_build(s + 1, vals, &t) < 0)
    return w.fail(JDS_EINVAL, "DHT %d/%d: BITS over-subscribe the code space", *tc, *th);
  return JDS_OK;
}

// The i-th component id of the SOS at hand (ns components) as the info counts
// them, from 1.  pre: what the walk puts in front of a scan's messages.
inline int hd_sos_component(const HdWalk& w, int i, int ns, const char* pre, int* comp) {
  int id = w.s[1 + 2 * i];
  if (w.ncomp == 1) {
    if (id != w.gray_id)
      return w.fail(JDS_EINVAL, "%sSOS names component %d, the grayscale frame's component is %d", pre, id, w.gray_id);
    id = 1;  // (the file's own id stays in its header)
  }
  if (id < 1 || id > 3) return w.fail(JDS_EINVAL, "%sSOS names component %d", pre, id);
  if (ns == 3 && id != i + 1)
    return w.fail(JDS_ENOTSUP, "%sinterleaved scan whose components are not 1, 2, 3 in that order", pre);
  *comp = id;
  return JDS_OK;
}

// The entropy-coded bytes of scan `scan` behind the SOS at hand: from w.p (the
// scan's offset) up to the next marker (0xFF, then neither 0x00 nor a fill
// 0xFF) that is no RSTm; with a restart interval in effect the RSTm markers
// belong to the scan.  *nm (nullable): how many there are; in_order: the i-th must be
// RST(i & 7).  *end: where the walk goes on.
inline int hd_scan_end(const HdWalk& w, int scan, bool in_order, int64_t* end, int64_t* nm = nullptr) {
  const uint8_t* data = w.data;  // (locals: this loop sees every byte of the file)
  const int64_t len = w.len;
  int64_t e = w.p, n = 0;
  for (;;) {
    if (e + 1 >= len) return w.fail(JDS_EINVAL, "truncated scan data: EOI missing");
    if (data[e] == 0xFF && data[e + 1] != 0x00) {
      const int r = data[e + 1] - 0xD0;
      if (r < 0 || r > 7) break;
      if (!w.ri)
        return w.fail(JDS_EINVAL, "scan %d: restart marker RST%d without a restart interval (no DRI)", scan, r);
      if (in_order && r != (int)(n & 7))
        return w.fail(JDS_EINVAL, "scan %d: restart marker RST%d where RST%d belongs (DRI %d)", scan, r,
                       (int)(n & 7), w.ri);
      ++n;
      e += 2;
      continue;
    }
    ++e;
  }
  *end = e;
  if (nm) *nm = n;
  return JDS_OK;
}

// The components' quantisation tables in row-major order, as everything behind the parser reads them.
inline void hd_qtables(const HdWalk& w, jds_jpeg_info* out) {
  for (int c = 0; c < w.ncomp; ++c)
    for (int k = 0; k < 64; ++k) out->qtable[c][HD_ZZ[k]] = (double)w.qt[out->tq[c]][k];
}

// The baseline marker walk: SOI, segments up to EOI, with or without restart
// intervals.  Where a segment has two defects the order of its checks decides
// which one is reported, and the two profiles' orders differ on purpose (each
// keeps its own messages and return codes).
inline int hd_walk(const uint8_t* data, int64_t len, HdProfile prof, jds_jpeg_info* out, char* msg, size_t cap) {
  const bool own = prof == HD_OWN;
  if (!data || !out || len < 0) return hd_fail(msg, cap, JDS_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) return hd_fail(msg, cap, JDS_EINVAL, "not a JPEG file: SOI missing");
  HdWalk w{data, len, msg, cap};
  bool seen[4] = {false, false, false, false};
  int rc;
  for (;;) {
    if ((rc = hd_next(w))) return rc;
    if (w.m == 0xD9) break;  // EOI
    const int m = w.m, ri = w.ri;
    if (m == 0xC0) {
      if ((rc = hd_frame(w, "SOF0", own, out))) return rc;
    } else if (m == 0xC4) {
      int tc, th, nv;
      for (int64_t q = 0; q < w.sl; q += 17 + nv) {
        if ((rc = hd_dht_table(w, q, 1, out->n_scans ? out->huff : nullptr, &tc, &th, &nv))) return rc;
        jds_jfif_huff* h = &out->huff[2 * tc + th];
        memset(h, 0, sizeof *h);
        memcpy(h->bits, w.s + q + 1, 16);
        memcpy(h->vals, w.s + q + 17, (size_t)nv);
        h->n_vals = nv;
        h->defined = 1;
      }
    } else if (m == 0xDA) {
      if (!w.sof) return hd_fail(msg, cap, JDS_EINVAL, "SOS before SOF0");
      if (w.sl < 1) return hd_fail(msg, cap, JDS_EINVAL, "SOS too short");
      const int ns = w.s[0];
      jds_jpeg_scan cur;  // (joins out->scan once every check has passed)
      memset(&cur, 0, sizeof cur);
      // the checks of an SOS, each written once; the profiles run them in their own orders below
      auto length = [&] {
        return w.sl != 4 + 2 * ns ? hd_fail(msg, cap, JDS_EINVAL, "SOS length does not match its component count") : 0;
      };
      auto count = [&] { return out->n_scans >= 3 ? hd_fail(msg, cap, JDS_EINVAL, "more than three scans") : 0; };
      auto spectral = [&] {
        const uint8_t* t = w.s + 1 + 2 * ns;
        return t[0] != 0 || t[1] != 63 || t[2] != 0
                   ? hd_fail(msg, cap, JDS_ENOTSUP, "spectral selection / successive approximation (progressive scan parameters)")
                   : 0;
      };
      auto component = [&](int i) {
        int comp;
        const int r = hd_sos_component(w, i, ns, "", &comp);
        if (r) return r;
        if (seen[comp]) return hd_fail(msg, cap, JDS_ENOTSUP, "component %d has a second scan", comp);
        cur.component[i] = comp;
        return 0;
      };
      auto tables = [&](int i) {
        const int td = w.s[2 + 2 * i] >> 4, ta = w.s[2 + 2 * i] & 15, tq = out->tq[cur.component[i] - 1];
        if (td > 1 || ta > 1) return hd_fail(msg, cap, JDS_EINVAL, "SOS table ids %d/%d", td, ta);
        if (!out->huff[td].defined || !out->huff[2 + ta].defined)
          return hd_fail(msg, cap, JDS_EINVAL, "SOS refers to a Huffman table the file has not defined");
        if (!w.qdef[tq]) return hd_fail(msg, cap, JDS_EINVAL, "quantisation table %d is not defined", tq);
        cur.dc_table[i] = td;
        cur.ac_table[i] = ta;
        return 0;
      };
      if (own) {
        if (ns != 1) return hd_fail(msg, cap, JDS_ENOTSUP, "interleaved scan (Ns = %d): non-interleaved scans only", ns);
        if ((rc = length()) || (rc = component(0)) || (rc = spectral()) || (rc = tables(0)) || (rc = count())) return rc;
      } else {
        if (w.ncomp == 1 && ns != 1)
          return hd_fail(msg, cap, JDS_EINVAL, "scan of %d components in a grayscale (one-component) frame", ns);
        if (w.ncomp == 1 && out->n_scans)
          return hd_fail(msg, cap, JDS_ENOTSUP, "a second scan in a grayscale (one-component) file");
        if (ns == 2)
          return hd_fail(msg, cap, JDS_ENOTSUP, "interleaved scan of two components (Ns = 2): one scan of three or three of one only");
        if (ns != 1 && ns != 3) return hd_fail(msg, cap, JDS_EINVAL, "SOS with %d components", ns);
        if ((rc = length())) return rc;
        if (out->interleaved || (ns == 3 && out->n_scans))
          return hd_fail(msg, cap, JDS_ENOTSUP, "a mix of interleaved and non-interleaved scans");
        if ((rc = count())) return rc;
        for (int i = 0; i < ns; ++i)
          if ((rc = component(i)) || (rc = tables(i))) return rc;
        if ((rc = spectral())) return rc;
      }
      // the entropy-coded segment; its RSTm markers are counted here and must come in order
      int64_t e, nm;
      if ((rc = hd_scan_end(w, out->n_scans, true, &e, &nm))) return rc;
      if (ri) {
        // the scan's MCUs: T.81's; own: the reference's block counts, the same number where they exist
        int64_t ny = 0, nc = 0;
        if (own && (rc = hd_block_counts(out->H, out->W, out->subsampling, &ny, &nc, msg, cap))) return rc;
        const int c0 = cur.component[0] - 1;
        const int64_t nmcu = ns == 3 ? out->mcu_cols * out->mcu_rows : out->grid_cols[c0] * out->grid_rows[c0];
        const int64_t need = (nmcu + ri - 1) / ri - 1;
        if (nm != need)
          return hd_fail(msg, cap, JDS_EINVAL, "scan %d: %lld restart markers where DRI %d needs %lld", out->n_scans,
                         (long long)nm, ri, (long long)need);
        if (data[e + 1] == 0xFF)
          return hd_fail(msg, cap, JDS_ENOTSUP, "scan %d: fill bytes (FF FF) in scan data with a restart interval (DRI %d)",
                         out->n_scans, ri);
      }
      for (int i = 0; i < ns; ++i) seen[cur.component[i]] = true;
      cur.n_components = ns;
      cur.restart_interval = ri;
      cur.offset = w.p;
      cur.length = e - cur.offset;
      out->scan[out->n_scans++] = cur;
      out->interleaved = ns == 3;
      w.p = e;
    } else {
      return hd_refuse_sof(w, "baseline SOF0 only");
    }
  }
  if (!w.sof) return hd_fail(msg, cap, JDS_EINVAL, "no SOF0 segment");
  if (out->n_scans != (out->interleaved || w.ncomp == 1 ? 1 : 3))
    return hd_fail(msg, cap, JDS_EINVAL, "%d scans (%s expected)", out->n_scans,
                   own ? "one per component" : "one interleaved scan or one per component");
  hd_qtables(w, out);
  int64_t ny = 0, nc = 0;
  return own ? hd_block_counts(out->H, out->W, out->subsampling, &ny, &nc, msg, cap) : JDS_OK;
}

inline int hd_jpeg_parse(const uint8_t* data, int64_t len, jds_jpeg_info* out, char* msg, size_t cap) {
  return hd_walk(data, len, HD_ANY, out, msg, cap);
}

// An own-profile file's info (hd_walk under HD_OWN) as the older public struct
// (include/jds.h: jds_jfif_parse): every scan has one component, one quantisation
// table serves all, and the grids of components 0 and 1 are the reference's block counts.
inline void jfif_info_of(const jds_jpeg_info* j, jds_jfif_info* out) {
  memset(out, 0, sizeof *out);
  out->H = j->H;
  out->W = j->W;
  out->subsampling = j->subsampling;
  out->n_scans = j->n_scans;
  memcpy(out->qtable, j->qtable[0], sizeof out->qtable);
  for (int i = 0; i < j->n_scans; ++i) {
    const jds_jpeg_scan& s = j->scan[i];
    out->scan[i] = {s.component[0], s.dc_table[0], s.ac_table[0], s.restart_interval, s.offset, s.length};
  }
  memcpy(out->huff, j->huff, sizeof out->huff);
  out->y_blocks = j->grid_cols[0] * j->grid_rows[0];
  out->c_blocks = j->grid_cols[1] * j->grid_rows[1];
  out->coeffs_needed = j->coeffs_needed;
  out->status = j->status;
  out->rounds = j->rounds;
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

// The next RSTm marker of n bytes of scan data at or after byte a (n: none).
inline long long next_rst(const uint8_t* d, long long a, long long n) {
  while (a < n) {
    const uint8_t* p = (const uint8_t*)memchr(d + a, 0xFF, (size_t)(n - a));
    if (!p) break;
    const long long e = p - d;
    if (e + 1 < n && d[e + 1] >= 0xD0 && d[e + 1] <= 0xD7) return e;
    a = e + 1;
  }
  return n;
}

// ------------------------------------------------------- host decode model --

struct HdHostSink {
  int16_t* out;
  void operator()(int64_t blk, int k, int v) const { out[blk * 64 + HD_ZZ[k]] = (int16_t)v; }
};

// The rounds and the write pass of one scan on the host, a loop standing in for
// the lanes, for any table choice and sink: subsequences of S bits, the
// propagation rule of the kernels (entry[i + 1] <- exit[i], changed entries
// decode again), block prefix, write pass.  The caller zeroes the output and
// sums the DC differences.  *rounds = decode rounds run.  Returns status bits.
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

// One non-interleaved scan without restart intervals: hd_host_sync, then the
// DC prefix sum.  out: nblocks x 64, zeroed here.
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

// The restart intervals of n bytes of scan data, a loop standing in for the
// lanes of k_dec_rst: the parser checked the markers' number and order, so
// interval i lies between markers i - 1 and i.  lane(bytes, nbytes, blk0, nb)
// decodes the interval of nb blocks from block blk0 on and returns status bits.
template <class Lane>
inline uint32_t hd_host_intervals(const uint8_t* d, int64_t n, int64_t ri, int64_t nblocks, Lane&& lane) {
  uint32_t st = 0;
  int64_t a = 0, blk0 = 0;
  while (blk0 < nblocks) {
    const int64_t e = next_rst(d, a, n);
    const int64_t nb = nblocks - blk0 < ri ? nblocks - blk0 : ri;
    st |= lane(d + a, e - a, blk0, nb);
    blk0 += nb;
    if (e >= n) break;
    a = e + 2;
  }
  if (blk0 < nblocks) st |= HD_RESTART;  // (the parser's marker count rules this out)
  return st;
}

// One non-interleaved scan with restart interval ri.  out: nblocks x 64, zeroed here.
inline uint32_t hd_host_scan_rst(const uint8_t* d, int64_t n, const HuffDecTab* dc, const HuffDecTab* ac, int64_t ri,
                                 int64_t nblocks, int16_t* out) {
  memset(out, 0, sizeof(int16_t) * 64 * (size_t)nblocks);
  return hd_host_intervals(d, n, ri, nblocks, [&](const uint8_t* b, int64_t nbytes, int64_t blk0, int64_t nb) {
    HdRstHostSink sink{out};
    const uint32_t st = hd_rst_lane(HdMemSrc{b, nbytes}, HdPlain{dc, ac}, blk0, nb, sink);
    return st | (sink.bad ? (uint32_t)HD_DC_RANGE : 0u);
  });
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

// A whole parsed file on the host (jds_selftest_huffdec / _jpegdec,
// tools/jfif_host_san.cpp): non-interleaved scans over their components' T.81
// grids (every restart interval a stream of its own: no propagation rounds),
// an interleaved one with the lanes' rules: intervals of at most lane_max
// blocks one lane each, longer ones (and a scan without intervals) through the
// rounds.  coeffs: info->coeffs_needed int16.  rounds[3]: per scan in file order.
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
  return hd_host_intervals(d, n, rib, nblocks, [&](const uint8_t* b, int64_t nbytes, int64_t blk0, int64_t nb) {
    if (rib <= lane_max) {
      HdIlRstSink sink{&m, coeffs, HD_ZZ, blk0};
      const uint32_t s1 = hd_rst_lane(HdMemSrc{b, nbytes}, tc, 0, nb, sink);
      return s1 | (sink.bad ? (uint32_t)HD_DC_RANGE : 0u);
    }
    int32_t r = 0;
    const uint32_t s2 = hd_host_sync(b, nbytes, tc, S, nb, HdIlSink{&m, coeffs, dcs.data(), HD_ZZ, blk0}, &r);
    rounds[0] = r > rounds[0] ? r : rounds[0];
    return s2 | hd_host_dc_mcu(&m, dcs.data(), blk0, blk0 + nb, coeffs);
  });
}

}  // namespace jds
