// jds_pjpeg_parse.hpp — the header parser of progressive files, the chain
// builder and the host model of their decode (DESIGN.md "Progressive files").
//
// Host only and HIP-free, on the marker walk of jds_jpeg_parse.hpp: the C-ABI
// (jds_abi_pjpeg.hip) and the stand-alone sanitizer program
// (tools/pjpeg_san.cpp) compile it; the lane routine it drives is the kernel's
// (jds_pjpeg_dec.hpp).
#pragma once
#include <vector>

#include "jds_jpeg_parse.hpp"
#include "jds_pjpeg_dec.hpp"

namespace jds {

// SOI, segments up to EOI.  Never reads outside [data, data + len).
inline int hd_pjpeg_parse(const uint8_t* data, int64_t len, jds_pjpeg_info* out, char* msg, size_t cap) {
  if (!data || !out || len < 0) return hd_fail(msg, cap, JDS_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  jds_jpeg_info* fr = &out->frame;
  if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) return hd_fail(msg, cap, JDS_EINVAL, "not a JPEG file: SOI missing");
  uint8_t qt[4][64];
  bool qdef[4] = {false, false, false, false};
  int64_t dht[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};  // the definitions in effect: offset of the Tc/Th byte
  int8_t last_al[3][64];  // per coefficient: the Al last coded; -1: not coded yet
  memset(last_al, -1, sizeof last_al);
  bool sof = false;
  int ri = 0, ncomp = 3, gray_id = 0;
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
      return hd_fail(msg, cap, JDS_ENOTSUP, "not progressive (SOF0): use the jpeg_* calls");
    } else if (m == 0xC2) {
      // the frame header, by the checks of the baseline parser's SOF0
      if (sof) return hd_fail(msg, cap, JDS_EINVAL, "second SOF2");
      if (sl < 6) return hd_fail(msg, cap, JDS_EINVAL, "SOF2 too short");
      if (s[0] != 8) return hd_fail(msg, cap, JDS_ENOTSUP, "sample precision %d (12-bit and other depths are not supported)", s[0]);
      fr->H = (s[1] << 8) | s[2];
      fr->W = (s[3] << 8) | s[4];
      const int nf = s[5];
      if (nf != 3 && nf != 1) return hd_fail(msg, cap, JDS_ENOTSUP, "%d components (one or three are supported)", nf);
      if (sl != 6 + 3 * nf) return hd_fail(msg, cap, JDS_EINVAL, "SOF2 length does not match its component count");
      if (fr->H < 1 || fr->W < 1)
        return hd_fail(msg, cap, JDS_ENOTSUP, "frame size %lldx%lld (DNL is not supported)", (long long)fr->H, (long long)fr->W);
      if (nf == 1) {
        const int h1 = s[7] >> 4, v1 = s[7] & 15;
        if (h1 < 1 || h1 > 4 || v1 < 1 || v1 > 4) return hd_fail(msg, cap, JDS_EINVAL, "sampling factors %dx%d (1..4 each)", h1, v1);
        ncomp = 1;
        gray_id = s[6];
        fr->subsampling = JDS_SS_GRAY;
      } else {
        for (int c = 0; c < 3; ++c)
          if (s[6 + 3 * c] != c + 1) return hd_fail(msg, cap, JDS_ENOTSUP, "component ids other than 1, 2, 3");
        const int ys = s[7];
        if (ys != 0x11 && ys != 0x21 && ys != 0x22)
          return hd_fail(msg, cap, JDS_ENOTSUP, "luma sampling %dx%d (1x1, 2x1 and 2x2 are supported)", ys >> 4, ys & 15);
        if (s[10] != 0x11 || s[13] != 0x11) return hd_fail(msg, cap, JDS_ENOTSUP, "subsampled or oversampled chroma factors");
        fr->subsampling = ys == 0x11 ? JDS_SS_444 : (ys == 0x21 ? JDS_SS_422 : JDS_SS_420);
      }
      const int hmax = ncomp == 1 ? 1 : s[7] >> 4, vmax = ncomp == 1 ? 1 : s[7] & 15;
      for (int c = 0; c < ncomp; ++c) {
        fr->tq[c] = s[8 + 3 * c];
        if (fr->tq[c] > 3) return hd_fail(msg, cap, JDS_EINVAL, "quantisation table id %d", fr->tq[c]);
        fr->hs[c] = c ? 1 : hmax;
        fr->vs[c] = c ? 1 : vmax;
        const int64_t xc = (fr->W * fr->hs[c] + hmax - 1) / hmax, yc = (fr->H * fr->vs[c] + vmax - 1) / vmax;
        fr->grid_cols[c] = (xc + 7) / 8;
        fr->grid_rows[c] = (yc + 7) / 8;
        fr->coeffs_needed += 64 * fr->grid_cols[c] * fr->grid_rows[c];
      }
      fr->single_table = ncomp == 1 || (fr->tq[0] == fr->tq[1] && fr->tq[0] == fr->tq[2]);
      fr->blocks_per_mcu = ncomp == 1 ? 1 : hmax * vmax + 2;
      fr->mcu_cols = (fr->W + 8 * hmax - 1) / (8 * hmax);
      fr->mcu_rows = (fr->H + 8 * vmax - 1) / (8 * vmax);
      int64_t ny = 0, nc = 0;
      fr->reference_grid = ncomp == 3 && hd_block_counts(fr->H, fr->W, fr->subsampling, &ny, &nc, nullptr, 0) == JDS_OK;
      fr->interleaved = ncomp == 3;
      fr->n_scans = 1;
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8) {
      if (m == 0xCC || m >= 0xC9) return hd_fail(msg, cap, JDS_ENOTSUP, "arithmetic coding (marker 0x%02X) is not supported", m);
      return hd_fail(msg, cap, JDS_ENOTSUP, "this frame type (SOF%d) is not supported: progressive SOF2 only", m - 0xC0);
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
        int nv = 0;
        for (int i = 0; i < 16; ++i) nv += s[q + 1 + i];
        if (nv > 256) return hd_fail(msg, cap, JDS_EINVAL, "DHT: BITS sum to %d symbols (more than 256)", nv);
        if (q + 17 + nv > sl) return hd_fail(msg, cap, JDS_EINVAL, "truncated DHT");
        uint8_t vals[256];
        memset(vals, 0, sizeof vals);
        memcpy(vals, s + q + 17, (size_t)nv);
        HuffDecTab t;
        if (hd_build(s + q + 1, vals, &t) < 0)
          return hd_fail(msg, cap, JDS_EINVAL, "DHT %d/%d: BITS over-subscribe the code space", tc, th);
        dht[tc][th] = (s + q) - data;
        q += 17 + nv;
      }
    } else if (m == 0xDA) {
      const int si = out->n_scans;
      if (!sof) return hd_fail(msg, cap, JDS_EINVAL, "SOS before SOF2");
      if (si >= JDS_PJPEG_MAX_SCANS)
        return hd_fail(msg, cap, JDS_ENOTSUP, "more than %d scans", JDS_PJPEG_MAX_SCANS);
      if (sl < 1) return hd_fail(msg, cap, JDS_EINVAL, "SOS too short");
      const int ns = s[0];
      if (ns < 1 || ns > 4) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS with %d components", si, ns);
      if (sl != 4 + 2 * ns) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS length does not match its component count", si);
      jds_pjpeg_scan cur;
      memset(&cur, 0, sizeof cur);
      const uint8_t* t = s + 1 + 2 * ns;
      cur.ss = t[0];
      cur.se = t[1];
      cur.ah = t[2] >> 4;
      cur.al = t[2] & 15;
      if (cur.ss > cur.se || cur.se > 63) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: spectral selection %d..%d", si, cur.ss, cur.se);
      if (cur.ss == 0 && cur.se != 0)
        return hd_fail(msg, cap, JDS_EINVAL, "scan %d: a progressive scan holds DC (0..0) or AC (1..63) coefficients, not %d..%d", si,
                       cur.ss, cur.se);
      if (cur.al > 13) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: successive approximation Al = %d (0..13)", si, cur.al);
      if (cur.ah != 0 && cur.al != cur.ah - 1)
        return hd_fail(msg, cap, JDS_EINVAL, "scan %d: successive approximation Ah = %d, Al = %d (a refinement has Al = Ah - 1)", si,
                       cur.ah, cur.al);
      if (cur.ss > 0 && ns != 1) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: AC scan with Ns = %d (an AC scan has one component)", si, ns);
      if (ncomp == 1 && ns != 1)
        return hd_fail(msg, cap, JDS_EINVAL, "scan %d: %d components in a grayscale (one-component) frame", si, ns);
      if (ns != 1 && ns != 3)
        return hd_fail(msg, cap, JDS_ENOTSUP, "scan %d: interleaved scan of %d components: one or all three only", si, ns);
      for (int i = 0; i < ns; ++i) {
        int comp = s[1 + 2 * i];
        if (ncomp == 1) {
          if (comp != gray_id)
            return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS names component %d, the grayscale frame's component is %d", si, comp, gray_id);
          comp = 1;
        }
        if (comp < 1 || comp > 3) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS names component %d", si, comp);
        if (ns == 3 && comp != i + 1)
          return hd_fail(msg, cap, JDS_ENOTSUP, "scan %d: interleaved scan whose components are not 1, 2, 3 in that order", si);
        const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
        if (td > 3 || ta > 3) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS table ids %d/%d", si, td, ta);
        cur.component[i] = comp;
        cur.dc_table[i] = td;
        cur.ac_table[i] = ta;
        cur.dc_dht[i] = cur.ac_dht[i] = -1;
        if (cur.ss == 0 && cur.ah == 0) cur.dc_dht[i] = dht[0][td];
        if (cur.ss > 0) cur.ac_dht[i] = dht[1][ta];
        if ((cur.ss == 0 && cur.ah == 0 && cur.dc_dht[i] < 0) || (cur.ss > 0 && cur.ac_dht[i] < 0))
          return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS refers to a Huffman table the file has not defined", si);
        if (!qdef[fr->tq[comp - 1]]) return hd_fail(msg, cap, JDS_EINVAL, "quantisation table %d is not defined", fr->tq[comp - 1]);
        // the progression of this component's band
        int8_t* la = last_al[comp - 1];
        if (cur.ss > 0 && la[0] < 0) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: AC scan before the component's first DC scan", si);
        for (int k = cur.ss; k <= cur.se; ++k) {
          if (cur.ah == 0 && la[k] >= 0)
            return hd_fail(msg, cap, JDS_EINVAL, "scan %d: coefficient %d has a second first pass (Ah = 0)", si, k);
          if (cur.ah != 0 && la[k] < 0)
            return hd_fail(msg, cap, JDS_EINVAL, "scan %d: refinement of coefficient %d before its first pass", si, k);
          if (cur.ah != 0 && la[k] != cur.ah)
            return hd_fail(msg, cap, JDS_EINVAL, "scan %d: Ah = %d where coefficient %d was last coded to Al = %d", si, cur.ah, k, la[k]);
        }
        for (int k = cur.ss; k <= cur.se; ++k) la[k] = (int8_t)cur.al;
      }
      // entropy-coded segment: up to the next marker that is no RSTm; the markers' number and
      // order are the decode's business (a wrong one is a defect of the scan data)
      int64_t e = p + 2 + ln;
      for (;;) {
        if (e + 1 >= len) return hd_fail(msg, cap, JDS_EINVAL, "truncated scan data: EOI missing");
        if (data[e] == 0xFF && data[e + 1] != 0x00) {
          const int r = data[e + 1] - 0xD0;
          if (r < 0 || r > 7) break;
          if (!ri) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: restart marker RST%d without a restart interval (no DRI)", si, r);
          e += 2;
          continue;
        }
        ++e;
      }
      cur.n_components = ns;
      cur.restart_interval = ri;
      cur.offset = p + 2 + ln;
      cur.length = e - cur.offset;
      out->scan[out->n_scans++] = cur;
      p = e;
      continue;
    }
    p += 2 + ln;
  }
  if (!sof) return hd_fail(msg, cap, JDS_EINVAL, "no SOF2 segment");
  if (out->n_scans < 1) return hd_fail(msg, cap, JDS_EINVAL, "no scan");
  for (int c = 0; c < ncomp; ++c)
    for (int k = 0; k < 64; ++k) fr->qtable[c][HD_ZZ[k]] = (double)qt[fr->tq[c]][k];
  out->complete = 1;
  for (int c = 0; c < ncomp; ++c)
    for (int k = 0; k < 64; ++k)
      if (last_al[c][k] != 0) out->complete = 0;
  return JDS_OK;
}

// The chains of a parsed file: one of all DC scans, one of each component's AC
// scans (a chain without scans is left out), their scans and decode tables
// appended to the batch's arrays.  file: the chain's MCU record and status
// word; data_off: the file's first byte in the source.  False: a table's BITS
// over-subscribe the code space (the parser refuses such a file).
inline bool pj_build_chains(const uint8_t* data, const jds_pjpeg_info* info, int file, long long data_off,
                            std::vector<PjChain>& chains, std::vector<PjScan>& scans, std::vector<HuffDecTab>& tabs) {
  const int ncomp = info->frame.subsampling == JDS_SS_GRAY ? 1 : 3;
  for (int ch = 0; ch <= ncomp; ++ch) {  // 0: DC; 1 + c: the AC scans of component c
    PjChain pc{file, (int32_t)scans.size(), 0, 0};
    for (int i = 0; i < info->n_scans; ++i) {
      const jds_pjpeg_scan& s = info->scan[i];
      if (ch == 0 ? s.ss != 0 : (s.ss == 0 || s.component[0] != ch)) continue;
      PjScan d;
      memset(&d, 0, sizeof d);
      d.data_off = data_off + s.offset;
      d.nbytes = s.length;
      d.ns = s.n_components;
      d.ss = s.ss;
      d.se = s.se;
      d.ah = s.ah;
      d.al = s.al;
      d.ri = s.restart_interval;
      for (int j = 0; j < 3; ++j) {
        d.comp[j] = j < s.n_components ? s.component[j] - 1 : 0;
        d.tab[j] = -1;
        const int64_t off = j < s.n_components ? (s.ss == 0 ? s.dc_dht[j] : s.ac_dht[j]) : -1;
        if (off < 0) continue;
        int nv = 0;
        for (int k = 0; k < 16; ++k) nv += data[off + 1 + k];
        uint8_t vals[256];
        memset(vals, 0, sizeof vals);
        memcpy(vals, data + off + 17, (size_t)(nv > 256 ? 256 : nv));
        HuffDecTab t;
        if (hd_build(data + off + 1, vals, &t) < 0) return false;
        d.tab[j] = (int32_t)tabs.size();
        tabs.push_back(t);
      }
      scans.push_back(d);
      ++pc.nscans;
    }
    if (pc.nscans) chains.push_back(pc);
  }
  return true;
}

// A parsed file on the host, chain after chain (jds_selftest_pjpegdec,
// tools/pjpeg_san.cpp).  coeffs: info->frame.coeffs_needed int16, zeroed here.
inline uint32_t hd_pjpeg_host_decode(const uint8_t* data, int64_t len, const jds_pjpeg_info* info, int16_t* coeffs) {
  std::vector<PjChain> chains;
  std::vector<PjScan> scans;
  std::vector<HuffDecTab> tabs;
  if (!pj_build_chains(data, info, 0, 0, chains, scans, tabs)) return HD_BAD_HEADER;
  memset(coeffs, 0, sizeof(int16_t) * (size_t)info->frame.coeffs_needed);
  const HdMcu m = hd_jpeg_mcu(&info->frame);
  const HdMemSrc src{data, len};
  uint32_t st = 0;
  for (const PjChain& c : chains)
    st |= hd_pjpeg_chain(src, tabs.data(), scans.data() + c.scan0, c.nscans, m, PjCoefSink{coeffs});
  return st;
}

}  // namespace jds
