// jds_abi_pjpeg.hip — the C-ABI's progressive-file calls (include/jds.h
// "Progressive files"; DESIGN.md "Progressive files"): parse, the chain decode,
// and behind it the existing batch renderings and the existing interleaved-scan
// writer, which take the decoded coefficients as they take a baseline file's.
//
// Host side only: descriptors (jds_pjpeg_parse.hpp), uploads and launches.
#include <string>

#include "jds_abi.hpp"
#include "jds_abi_jpeg.hpp"
#include "jds_jpeg_ljs.hpp"
#include "jds_pjpeg_parse.hpp"

namespace jds {
hipError_t launch_pjpeg_chains(const uint8_t* files, long long files_bytes, const PjChain* chains, int nchains,
                               const PjScan* scans, const HuffDecTab* tabs, const HdMcu* mcus, int16_t* coeffs,
                               uint32_t* status, unsigned long long* ticks, hipStream_t s);
}

extern "C" {

static int pj_parse_file(const uint8_t* data, int64_t len, jds_pjpeg_info* out) {
  const int rc = hd_pjpeg_parse(data, len, out, g_err, sizeof g_err);
  if (rc) return rc;
  if (out->frame.H * out->frame.W > (int64_t)1 << 28)
    return fail(JDS_EINVAL, "unsupported image size %lldx%lld", (long long)out->frame.H, (long long)out->frame.W);
  return JDS_OK;
}

int jds_pjpeg_parse(const uint8_t* data, int64_t len, jds_pjpeg_info* out) { return pj_parse_file(data, len, out); }

static int pj_coef_cap(const int16_t* coeffs, int64_t cap, int64_t needed) {
  if (!coeffs || cap < needed)
    return fail(JDS_EINVAL, "coefficient buffer too small: %lld entries needed", (long long)needed);
  return JDS_OK;
}

int jds_selftest_pjpegdec(const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap, jds_pjpeg_info* info) {
  if (!info) return fail(JDS_EINVAL, "null argument");
  int rc;
  if ((rc = pj_parse_file(data, len, info)) || (rc = pj_coef_cap(coeffs, coeffs_cap, info->frame.coeffs_needed))) return rc;
  const uint32_t st = hd_pjpeg_host_decode(data, len, info, coeffs);
  info->status = info->frame.status = st;
  if (st) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(st), st);
  return JDS_OK;
}

// What the layout keeps per batch (jds_abi_jpeg.hip: BatchPlan).
struct PjPlan {
  std::vector<jds_pjpeg_info> info;  // per file
  std::vector<int> rec_of;           // per file: its record, or -1
  std::vector<int> file_of;          // per record: its file
  std::vector<JInvRec> recs;
  std::vector<JInvMap> map[JI_MODES];
  std::vector<JInvMap> smap[JI_MODES][LS_ND];
  bool any_scaled = false;
  int64_t rgb_bytes = 0, coef_entries = 0;
  int first_bad = -1;
  char first_msg[400] = "";
  void bad(int i, const char* m) {
    if (first_bad < 0 || i < first_bad) {
      first_bad = i;
      snprintf(first_msg, sizeof first_msg, "%s", m);
    }
  }
};

// batch_layout (jds_abi_jpeg.hip) for progressive files.  render_it: the files
// are rendered, so an incomplete progression is an item error.
static int pj_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items, PjPlan& bp,
                     bool render_it, int32_t render, const int32_t* denoms, jds_jpeg_scaled_item* scaled) {
  if (n < 0 || (n > 0 && (!data || !lens || !items))) return fail(JDS_EINVAL, "null argument");
  for (int i = 0; denoms && i < n; ++i) {
    if (!ls_denom_ok(denoms[i])) return fail(JDS_EINVAL, "file %d: scale_denom %d is not 1, 2, 4 or 8", i, (int)denoms[i]);
    const int rc = scale_check(render, denoms[i]);
    if (rc) return rc;
  }
  bp.info.resize((size_t)n);
  bp.rec_of.assign((size_t)n, -1);
  std::vector<JInvRec> parsed((size_t)n);
  std::vector<std::string> msg((size_t)n);
  batch_parallel(n, [&](int i) {
    jds_jpeg_batch_item& it = items[i];
    memset(&it, 0, sizeof it);
    it.rgb_off = -1;
    it.coef_off = -1;
    jds_pjpeg_info& info = bp.info[(size_t)i];
    JInvRec& r = parsed[(size_t)i];
    memset(&r, 0, sizeof r);
    int rc = data[i] && lens[i] >= 0 ? pj_parse_file(data[i], lens[i], &info) : fail(JDS_EINVAL, "null file");
    if (rc == JDS_OK) {
      it.H = info.frame.H;
      it.W = info.frame.W;
      it.subsampling = info.frame.subsampling;
      it.interleaved = info.frame.interleaved;
      rc = jpeg_inv_args(&info.frame, &r.a);
    }
    if (rc == JDS_OK && render_it && !info.complete)
      rc = fail(JDS_ENOTSUP, "incomplete progression: the scans do not code every coefficient down to Al = 0");
    it.rc = rc;
    if (rc != JDS_OK) msg[(size_t)i] = g_err;
  });
  for (int i = 0; i < n; ++i) {
    jds_jpeg_batch_item& it = items[i];
    JInvRec& r = parsed[(size_t)i];
    if (it.rc != JDS_OK) {
      bp.bad(i, msg[(size_t)i].c_str());
      continue;
    }
    long long rb = bp.rgb_bytes, ce = bp.coef_entries;
    const int dn = denoms ? denoms[i] : 1;
    ls_batch_place(r, (int)bp.recs.size(), dn, bp.info[(size_t)i].frame.coeffs_needed, &rb, &ce);
    bp.any_scaled = bp.any_scaled || dn != 1;
    bp.rgb_bytes = rb;
    bp.coef_entries = ce;
    it.rgb_off = r.rgb_off;
    it.coef_off = r.coef_off;
    it.coeffs_needed = bp.info[(size_t)i].frame.coeffs_needed;
    bp.rec_of[(size_t)i] = r.st;
    bp.file_of.push_back(i);
    bp.recs.push_back(r);
  }
  if (bp.coef_entries / 64 > 0x7fffffffll || !ls_batch_maps(bp.recs.data(), (int)bp.recs.size(), bp.map, bp.smap))
    return fail(JDS_ENOTSUP, "batch of %d files: too many blocks or tiles for one set of launches", n);
  for (int i = 0; scaled && i < n; ++i) {
    memset(&scaled[i], 0, sizeof scaled[i]);
    scaled[i].scale_denom = denoms ? denoms[i] : 1;
    if (items[i].rc != JDS_OK) continue;
    long long oh, ow;
    ls_scaled_size(items[i].H, items[i].W, scaled[i].scale_denom, &oh, &ow);
    scaled[i].out_h = oh;
    scaled[i].out_w = ow;
  }
  return JDS_OK;
}

static void pj_note(const PjPlan& bp) {
  if (bp.first_bad >= 0) {
    char m[400];
    snprintf(m, sizeof m, "%s", bp.first_msg);
    fail(0, "file %d: %s", bp.first_bad, m);
  } else {
    g_err[0] = 0;
  }
}

// The launches of a laid-out batch with at least one record: one upload, the
// coefficients zeroed (progressive decoding accumulates), k_pjpeg_chains into
// c->ent_cf (file k's coefficients at bp.recs[k].coef_off), then with
// `inverse` the batch rendering into rgb; the status words into items.
// Synchronous.
// cf_ext (nullable): the caller's device buffer of bp.coef_entries entries instead of c->ent_cf.
static int pj_run(jds_ctx* c, PjPlan& bp, const uint8_t* const* data, const int64_t* lens, uint8_t* rgb,
                  int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items, bool inverse, int32_t render,
                  int16_t* cf_ext = nullptr) {
  const int nv = (int)bp.recs.size();
  hipStream_t s = c->stream;
  HIP_TRY(hipSetDevice(c->device));
  auto up = [](size_t v, size_t a) { return (v + a - 1) / a * a; };
  std::vector<size_t> foff((size_t)nv);
  size_t o = 0;
  for (int k = 0; k < nv; ++k) {
    foff[(size_t)k] = o;
    o = up(o + (size_t)lens[bp.file_of[(size_t)k]], 16);
  }
  std::vector<PjChain> chains;
  std::vector<PjScan> scans;
  std::vector<HuffDecTab> tabs;
  std::vector<HdMcu> mcus((size_t)nv);
  std::vector<uint32_t> st0((size_t)nv, 0u);
  for (int k = 0; k < nv; ++k) {
    const int i = bp.file_of[(size_t)k];
    HdMcu m = hd_jpeg_mcu(&bp.info[(size_t)i].frame);
    for (int cc = 0; cc < 3; ++cc) m.off[cc] += bp.recs[(size_t)k].coef_off;
    mcus[(size_t)k] = m;
    if (!pj_build_chains(data[i], &bp.info[(size_t)i], k, (long long)foff[(size_t)k], chains, scans, tabs))
      return fail(JDS_EINVAL, "file %d: DHT: BITS over-subscribe the code space", i);  // (the parser has refused these)
  }
  if (chains.size() > 0x7fffffffull || scans.size() > 0x7fffffffull || tabs.size() > 0x7fffffffull)
    return fail(JDS_ENOTSUP, "batch too long for one decode");
  int map_off[JI_MODES], nmap[JI_MODES], tiles[JI_MODES], nm = 0;
  for (int m = 0; m < JI_MODES; ++m) {
    map_off[m] = nm;
    nmap[m] = (int)bp.map[m].size() - 1;
    tiles[m] = bp.map[m].back().tile0;
    nm += (int)bp.map[m].size();
  }
  int smap_off[JI_MODES][LS_ND], nsmap[JI_MODES][LS_ND], stiles[JI_MODES][LS_ND];
  for (int m = 0; m < JI_MODES; ++m)
    for (int d = 0; d < LS_ND; ++d) {
      smap_off[m][d] = nm;
      nsmap[m][d] = bp.any_scaled ? (int)bp.smap[m][d].size() - 1 : 0;
      stiles[m][d] = bp.any_scaled ? bp.smap[m][d].back().tile0 : 0;
      if (bp.any_scaled) nm += (int)bp.smap[m][d].size();
    }
  // the upload: every part at a 256-byte boundary, files at 16-byte ones inside theirs
  const size_t files_bytes = up(o, 256);
  const size_t o_files = 0, o_tabs = files_bytes, o_mcu = up(o_tabs + sizeof(HuffDecTab) * tabs.size(), 256),
               o_rec = up(o_mcu + sizeof(HdMcu) * mcus.size(), 256), o_map = up(o_rec + sizeof(JInvRec) * (size_t)nv, 256),
               o_scan = up(o_map + sizeof(JInvMap) * (size_t)nm, 256), o_chain = up(o_scan + sizeof(PjScan) * scans.size(), 256),
               o_st = up(o_chain + sizeof(PjChain) * chains.size(), 256), total = up(o_st + 4 * (size_t)nv, 256);
  if (total > c->bat_host_cap) {
    if (c->bat_host) (void)hipHostFree(c->bat_host);
    c->bat_host = nullptr;
    c->bat_host_cap = 0;
    HIP_TRY(hipHostMalloc(&c->bat_host, total, hipHostMallocDefault));
    c->bat_host_cap = total;
  }
  char* h = (char*)c->bat_host;
  batch_parallel(nv, [&](int k) {
    const int i = bp.file_of[(size_t)k];
    memcpy(h + o_files + foff[(size_t)k], data[i], (size_t)lens[i]);
  });
  if (!tabs.empty()) memcpy(h + o_tabs, tabs.data(), sizeof(HuffDecTab) * tabs.size());
  memcpy(h + o_mcu, mcus.data(), sizeof(HdMcu) * mcus.size());
  memcpy(h + o_rec, bp.recs.data(), sizeof(JInvRec) * (size_t)nv);
  for (int m = 0; m < JI_MODES; ++m)
    memcpy(h + o_map + sizeof(JInvMap) * (size_t)map_off[m], bp.map[m].data(), sizeof(JInvMap) * bp.map[m].size());
  for (int m = 0; bp.any_scaled && m < JI_MODES; ++m)
    for (int d = 0; d < LS_ND; ++d)
      memcpy(h + o_map + sizeof(JInvMap) * (size_t)smap_off[m][d], bp.smap[m][d].data(),
             sizeof(JInvMap) * bp.smap[m][d].size());
  if (!scans.empty()) memcpy(h + o_scan, scans.data(), sizeof(PjScan) * scans.size());
  if (!chains.empty()) memcpy(h + o_chain, chains.data(), sizeof(PjChain) * chains.size());
  memcpy(h + o_st, st0.data(), 4 * (size_t)nv);
  HIP_TRY(c->bat.ensure(total));
  if (!cf_ext) HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)bp.coef_entries));
  uint8_t* dst = rgb;
  if (inverse && !rgb_on_device) {
    HIP_TRY(c->out.ensure((size_t)bp.rgb_bytes));
    dst = (uint8_t*)c->out.p;
  }
  char* dv = (char*)c->bat.p;
  const CtxMarkScope marks_(c, s);
  HIP_TRY(hipMemcpyAsync(dv, h, total, hipMemcpyHostToDevice, s));
  int16_t* cf_d = cf_ext ? cf_ext : (int16_t*)c->ent_cf.p;
  HIP_TRY(hipMemsetAsync(cf_d, 0, sizeof(int16_t) * (size_t)bp.coef_entries, s));
  kmark(s, "(batch upload)");
  uint32_t* st_d = (uint32_t*)(dv + o_st);
  unsigned long long* ticks_d = nullptr;
  if (c->prof_on) {  // the walk time of every scan, for jds_pjpeg_scan_times
    HIP_TRY(c->pj_ticks.ensure(8 * scans.size()));
    ticks_d = (unsigned long long*)c->pj_ticks.p;
    HIP_TRY(hipMemsetAsync(ticks_d, 0, 8 * scans.size(), s));
  }
  HIP_TRY(launch_pjpeg_chains((const uint8_t*)(dv + o_files), (long long)files_bytes, (const PjChain*)(dv + o_chain),
                              (int)chains.size(), (const PjScan*)(dv + o_scan), (const HuffDecTab*)(dv + o_tabs),
                              (const HdMcu*)(dv + o_mcu), cf_d, st_d, ticks_d, s));
  if (inverse && render == JDS_RENDER_LIBJPEG)
    HIP_TRY(launch_jpeg_ljt_batch((const JInvRec*)(dv + o_rec), (const JInvMap*)(dv + o_map), map_off, nmap, tiles, st_d,
                                  cf_d, dst, s));
  else if (inverse)
    HIP_TRY(launch_jpeg_inv_batch((const JInvRec*)(dv + o_rec), (const JInvMap*)(dv + o_map), map_off, nmap, tiles, st_d,
                                  cf_d, dst, s));
  if (inverse && bp.any_scaled)
    HIP_TRY(launch_jpeg_ljs_batch((const JInvRec*)(dv + o_rec), (const JInvMap*)(dv + o_map), smap_off, nsmap, stiles,
                                  st_d, cf_d, dst, s));
  if (inverse && !rgb_on_device)  // image by image: the gaps of the caller's buffer stay as they are
    for (int k = 0; k < nv; ++k) {
      const JInvRec& r = bp.recs[(size_t)k];
      long long oh, ow;
      ls_scaled_size(r.a.H, r.a.W, ls_rec_denom(r), &oh, &ow);
      HIP_TRY(hipMemcpyAsync(rgb + r.rgb_off, dst + r.rgb_off, (size_t)oh * (size_t)ow * 3, hipMemcpyDeviceToHost, s));
    }
  if (coeffs)
    HIP_TRY(hipMemcpyAsync(coeffs, cf_d, sizeof(int16_t) * (size_t)bp.coef_entries, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(st0.data(), st_d, 4 * (size_t)nv, hipMemcpyDeviceToHost, s));
  kmark(s, "(batch download)");
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < nv; ++k) items[bp.file_of[(size_t)k]].status = st0[(size_t)k];
  c->pj_scan_us.clear();
  if (ticks_d) {
    std::vector<unsigned long long> t(scans.size());
    int khz = 0;
    HIP_TRY(hipMemcpy(t.data(), ticks_d, 8 * t.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    for (unsigned long long v : t) c->pj_scan_us.push_back(khz > 0 ? (double)v * 1e3 / khz : 0.0);
  }
  return JDS_OK;
}

int jds_pjpeg_scan_times(jds_ctx* c, double* us, int64_t cap, int64_t* count) {
  if (!c || !count) return fail(JDS_EINVAL, "null argument");
  *count = (int64_t)c->pj_scan_us.size();
  if (*count > cap || (*count && !us)) return fail(JDS_EINVAL, "%lld entries needed", (long long)*count);
  for (size_t i = 0; i < c->pj_scan_us.size(); ++i) us[i] = c->pj_scan_us[i];
  return JDS_OK;
}

int jds_pjpeg_batch_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items,
                           int64_t* rgb_bytes, int64_t* coef_entries, const int32_t* scale_denoms,
                           jds_jpeg_scaled_item* scaled) {
  if (!rgb_bytes || !coef_entries) return fail(JDS_EINVAL, "null argument");
  PjPlan bp;
  const int rc = pj_layout(data, lens, n, items, bp, true, JDS_RENDER_LIBJPEG, scale_denoms, scaled);
  if (rc) return rc;
  *rgb_bytes = bp.rgb_bytes;
  *coef_entries = bp.coef_entries;
  pj_note(bp);
  return JDS_OK;
}

int jds_pjpeg_batch_to_rgb(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                           int64_t rgb_cap, int32_t rgb_on_device, int32_t render, const int32_t* scale_denoms,
                           jds_jpeg_batch_item* items, jds_jpeg_scaled_item* scaled, int16_t* coeffs) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!c) return fail(JDS_EINVAL, "null argument");
  PjPlan bp;
  if ((rc = pj_layout(data, lens, n, items, bp, true, render, scale_denoms, scaled))) return rc;
  if (bp.rgb_bytes > 0 && (!rgb || rgb_cap < bp.rgb_bytes))
    return fail(JDS_EINVAL, "image buffer too small: %lld bytes needed", (long long)bp.rgb_bytes);
  if (!bp.recs.empty() && (rc = pj_run(c, bp, data, lens, rgb, rgb_on_device, coeffs, items, true, render))) return rc;
  pj_note(bp);
  return JDS_OK;
}

// A batch of one: the item's error, or its scan data's defect, is the call's.
static int pj_single_result(const jds_jpeg_batch_item& it, uint32_t status, jds_pjpeg_info* info) {
  info->status = info->frame.status = status;
  if (it.rc) {
    // ("file 0: <message>" -> the message)
    std::string m = g_err;
    if (m.rfind("file 0: ", 0) == 0) m = m.substr(8);
    return fail(it.rc, "%s", m.c_str());
  }
  if (status) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(status), status);
  return JDS_OK;
}

static int pj_decode(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap, bool on_device,
                     jds_pjpeg_info* info) {
  if (!c || !data || !info) return fail(JDS_EINVAL, "null argument");
  PjPlan bp;
  jds_jpeg_batch_item it;
  int rc;
  if ((rc = pj_layout(&data, &len, 1, &it, bp, false, JDS_RENDER_REFERENCE, nullptr, nullptr))) return rc;
  *info = bp.info[0];
  pj_note(bp);
  if (it.rc == JDS_OK) {
    if ((rc = pj_coef_cap(coeffs, coeffs_cap, info->frame.coeffs_needed))) return rc;
    if ((rc = pj_run(c, bp, &data, &len, nullptr, 0, on_device ? nullptr : coeffs, &it, false, JDS_RENDER_REFERENCE,
                     on_device ? coeffs : nullptr)))
      return rc;
  }
  return pj_single_result(it, it.status, info);
}

int jds_pjpeg_decode(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                     jds_pjpeg_info* info) {
  return pj_decode(c, data, len, coeffs, coeffs_cap, false, info);
}

int jds_pjpeg_decode_dev(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs_dev, int64_t coeffs_cap,
                         jds_pjpeg_info* info) {
  return pj_decode(c, data, len, coeffs_dev, coeffs_cap, true, info);
}

int jds_pjpeg_to_rgb(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                     int32_t rgb_on_device, int32_t render, int32_t scale_denom, int16_t* coeffs,
                     jds_pjpeg_info* info) {
  int rc;
  if ((rc = render_check(render)) || (rc = scale_check(render, scale_denom))) return rc;
  if (!c || !data || !info || !rgb_out) return fail(JDS_EINVAL, "null argument");
  PjPlan bp;
  jds_jpeg_batch_item it;
  if ((rc = pj_layout(&data, &len, 1, &it, bp, true, render, &scale_denom, nullptr))) return rc;
  *info = bp.info[0];
  pj_note(bp);
  if (it.rc == JDS_OK) {
    long long oh, ow;
    ls_scaled_size(it.H, it.W, scale_denom, &oh, &ow);
    if (rgb_cap < oh * ow * 3) return fail(JDS_EINVAL, "image buffer too small: %lld bytes needed", oh * ow * 3);
    if ((rc = pj_run(c, bp, &data, &len, rgb_out, rgb_on_device, coeffs, &it, true, render))) return rc;
  }
  return pj_single_result(it, it.status, info);
}

// The prefix of a transcoded progressive file: mcu_splice's (every segment before the first SOS
// except DHT and DRI), its SOF2 marker rewritten as SOF0.
static int pj_prefix(const uint8_t* data, int64_t len, McuJob* j) {
  const int64_t n = mcu_splice(data, len, nullptr, 0);
  if (n < 0 || n > 0x7fffffffll) return fail(JDS_EINVAL, "header splice: no marker sequence from SOI to an SOS");
  j->pfx.resize((size_t)n);
  if (mcu_splice(data, len, j->pfx.data(), n) != n) return fail(JDS_EINVAL, "header splice: length mismatch");
  int64_t p = 0;
  while (p + 4 <= n) {  // (whole segments, no fill bytes: the splicer wrote them)
    const int64_t ln = ((int64_t)j->pfx[(size_t)p + 2] << 8) | j->pfx[(size_t)p + 3];
    if (j->pfx[(size_t)p + 1] == 0xC2) j->pfx[(size_t)p + 1] = 0xC0;
    p += 2 + ln;
  }
  return JDS_OK;
}

int jds_pjpeg_batch_transcode(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, int32_t optimize,
                              uint8_t* out, int64_t out_cap, int32_t out_on_device, jds_jpeg_transcode_item* items,
                              int64_t* out_bytes) {
  if (!c || !out_bytes || (n > 0 && !items)) return fail(JDS_EINVAL, "null argument");
  *out_bytes = 0;
  std::vector<jds_jpeg_batch_item> bi((size_t)(n > 0 ? n : 0));
  PjPlan bp;
  int rc = pj_layout(data, lens, n, bi.data(), bp, false, JDS_RENDER_REFERENCE, nullptr, nullptr);
  if (rc) return rc;
  if (!bp.recs.empty() && (rc = pj_run(c, bp, data, lens, nullptr, 0, nullptr, bi.data(), false, JDS_RENDER_REFERENCE)))
    return rc;
  for (int i = 0; i < n; ++i) {
    jds_jpeg_transcode_item& it = items[i];
    memset(&it, 0, sizeof it);
    it.rc = bi[(size_t)i].rc;
    it.status = bi[(size_t)i].status;
    it.H = bi[(size_t)i].H;
    it.W = bi[(size_t)i].W;
    it.subsampling = bi[(size_t)i].subsampling;
    it.interleaved = bi[(size_t)i].interleaved;
    it.out_off = -1;
  }
  std::vector<McuJob> jobs;
  std::vector<int> job_file;
  for (size_t k = 0; k < bp.recs.size(); ++k) {
    const int i = bp.file_of[k];
    if (items[i].status || items[i].rc) continue;
    McuJob j;
    if ((rc = mcu_job_geo(&bp.info[(size_t)i].frame, bp.recs[k].coef_off, &j))) return rc;
    if ((rc = pj_prefix(data[i], lens[i], &j))) return rc;
    jobs.push_back(std::move(j));
    job_file.push_back(i);
  }
  if (jobs.empty()) {
    pj_note(bp);
    return JDS_OK;
  }
  const CtxMarkScope marks_(c, c->stream);
  rc = mcu_write_batch(c, jobs, job_file, optimize, nullptr, out, out_cap, out_on_device, items, out_bytes,
                       [&](int i, const char* m) { bp.bad(i, m); });
  if (rc) return rc;
  pj_note(bp);
  return JDS_OK;
}

int jds_pjpeg_transcode(jds_ctx* c, const uint8_t* data, int64_t len, int32_t optimize, uint8_t* out, int64_t out_cap,
                        int64_t* out_len, jds_pjpeg_info* info) {
  if (!c || !data || !info || !out_len) return fail(JDS_EINVAL, "null argument");
  int rc;
  if ((rc = pj_parse_file(data, len, info))) return rc;
  jds_jpeg_transcode_item it;
  memset(&it, 0, sizeof it);
  int64_t need = 0;
  rc = jds_pjpeg_batch_transcode(c, &data, &len, 1, optimize, out, out_cap, 0, &it, &need);
  info->status = info->frame.status = it.status;
  *out_len = rc && need > out_cap ? need : it.out_len;  // (too small: the batch's need, the length rounded up to 256)
  if (rc) return rc;
  if (it.rc) {
    std::string m = g_err;
    if (m.rfind("file 0: ", 0) == 0) m = m.substr(8);
    return fail(it.rc, "%s", m.c_str());
  }
  if (it.status) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(it.status), it.status);
  return JDS_OK;
}

}  // extern "C"
