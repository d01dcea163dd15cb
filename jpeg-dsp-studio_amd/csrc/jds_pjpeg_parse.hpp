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

// The progressive marker walk, on the pieces of the baseline one
// (jds_jpeg_parse.hpp); its own: the scan cap, the Ss/Se/Ah/Al checks, the DHT
// definitions in effect per scan, and the progression's bookkeeping.
inline int hd_pjpeg_parse(const uint8_t* data, int64_t len, jds_pjpeg_info* out, char* msg, size_t cap) {
  if (!data || !out || len < 0) return hd_fail(msg, cap, JDS_EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  jds_jpeg_info* fr = &out->frame;
  if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) return hd_fail(msg, cap, JDS_EINVAL, "not a JPEG file: SOI missing");
  int64_t dht[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};  // the definitions in effect: offset of the Tc/Th byte
  int8_t last_al[3][64];  // per coefficient: the Al last coded; -1: not coded yet
  memset(last_al, -1, sizeof last_al);
  HdWalk w{data, len, msg, cap};
  int rc;
  for (;;) {
    if ((rc = hd_next(w))) return rc;
    if (w.m == 0xD9) break;  // EOI
    const int m = w.m;
    if (m == 0xC0) {
      return hd_fail(msg, cap, JDS_ENOTSUP, "not progressive (SOF0): use the jpeg_* calls");
    } else if (m == 0xC2) {
      if ((rc = hd_frame(w, "SOF2", false, fr))) return rc;
      fr->interleaved = w.ncomp == 3;
      fr->n_scans = 1;
    } else if (m == 0xC4) {
      int tc, th, nv;
      for (int64_t q = 0; q < w.sl; q += 17 + nv) {
        if ((rc = hd_dht_table(w, q, 3, nullptr, &tc, &th, &nv))) return rc;
        dht[tc][th] = (w.s + q) - data;
      }
    } else if (m == 0xDA) {
      const int si = out->n_scans;
      if (!w.sof) return hd_fail(msg, cap, JDS_EINVAL, "SOS before SOF2");
      if (si >= JDS_PJPEG_MAX_SCANS)
        return hd_fail(msg, cap, JDS_ENOTSUP, "more than %d scans", JDS_PJPEG_MAX_SCANS);
      if (w.sl < 1) return hd_fail(msg, cap, JDS_EINVAL, "SOS too short");
      const int ns = w.s[0];
      if (ns < 1 || ns > 4) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS with %d components", si, ns);
      if (w.sl != 4 + 2 * ns) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS length does not match its component count", si);
      jds_pjpeg_scan cur;
      memset(&cur, 0, sizeof cur);
      char pre[24];
      snprintf(pre, sizeof pre, "scan %d: ", si);
      const uint8_t* t = w.s + 1 + 2 * ns;
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
      if (w.ncomp == 1 && ns != 1)
        return hd_fail(msg, cap, JDS_EINVAL, "scan %d: %d components in a grayscale (one-component) frame", si, ns);
      if (ns != 1 && ns != 3)
        return hd_fail(msg, cap, JDS_ENOTSUP, "scan %d: interleaved scan of %d components: one or all three only", si, ns);
      for (int i = 0; i < ns; ++i) {
        int comp;
        if ((rc = hd_sos_component(w, i, ns, pre, &comp))) return rc;
        const int td = w.s[2 + 2 * i] >> 4, ta = w.s[2 + 2 * i] & 15;
        if (td > 3 || ta > 3) return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS table ids %d/%d", si, td, ta);
        cur.component[i] = comp;
        cur.dc_table[i] = td;
        cur.ac_table[i] = ta;
        cur.dc_dht[i] = cur.ac_dht[i] = -1;
        if (cur.ss == 0 && cur.ah == 0) cur.dc_dht[i] = dht[0][td];
        if (cur.ss > 0) cur.ac_dht[i] = dht[1][ta];
        if ((cur.ss == 0 && cur.ah == 0 && cur.dc_dht[i] < 0) || (cur.ss > 0 && cur.ac_dht[i] < 0))
          return hd_fail(msg, cap, JDS_EINVAL, "scan %d: SOS refers to a Huffman table the file has not defined", si);
        if (!w.qdef[fr->tq[comp - 1]]) return hd_fail(msg, cap, JDS_EINVAL, "quantisation table %d is not defined", fr->tq[comp - 1]);
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
      // the entropy-coded segment; its RSTm markers' number and order are the decode's business
      // (a wrong one is a defect of the scan data)
      int64_t e;
      if ((rc = hd_scan_end(w, si, false, &e))) return rc;
      cur.n_components = ns;
      cur.restart_interval = w.ri;
      cur.offset = w.p;
      cur.length = e - cur.offset;
      out->scan[out->n_scans++] = cur;
      w.p = e;
    } else {
      return hd_refuse_sof(w, "progressive SOF2 only");
    }
  }
  if (!w.sof) return hd_fail(msg, cap, JDS_EINVAL, "no SOF2 segment");
  if (out->n_scans < 1) return hd_fail(msg, cap, JDS_EINVAL, "no scan");
  hd_qtables(w, fr);
  out->complete = 1;
  for (int c = 0; c < w.ncomp; ++c)
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
