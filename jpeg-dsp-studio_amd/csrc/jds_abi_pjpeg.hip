// jds_abi_pjpeg.hip — the C-ABI's progressive-file calls (include/jds.h
// "Progressive files"; DESIGN.md "Progressive files"): parse, the chain decode,
// and behind it the existing batch renderings and the existing interleaved-scan
// writer, which take the decoded coefficients as they take a baseline file's.
//
// Host side only: descriptors (jds_pjpeg_parse.hpp), uploads and launches.
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

// A batch of one (single_result, jds_abi_jpeg.hip), its status into both places of the info.
static int pj_single_result(int item_rc, uint32_t status, jds_pjpeg_info* info) {
  info->status = info->frame.status = status;
  return single_result(item_rc, status);
}

int jds_selftest_pjpegdec(const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap, jds_pjpeg_info* info) {
  if (!info) return fail(JDS_EINVAL, "null argument");
  int rc;
  if ((rc = pj_parse_file(data, len, info)) || (rc = check_coef_cap(coeffs, coeffs_cap, info->frame.coeffs_needed))) return rc;
  return pj_single_result(JDS_OK, hd_pjpeg_host_decode(data, len, info, coeffs), info);
}

// The progressive front end of the batch driver (jds_abi_jpeg.hpp): the plan
// keeps every file's frame, this keeps the scans beside it; the decode is one
// k_pjpeg_chains launch over every file's chains.
struct PjFront : BatchFront {
  std::vector<jds_pjpeg_info> info;  // per file
  std::vector<PjScan> scans;         // of the run
  unsigned long long* ticks_d = nullptr;  // their walk times on the device (a profiled context)
  // render_it: the files are rendered, so an incomplete progression is an item error.
  // cf_ext (nullable): the caller's device buffer of the plan's coef_entries instead of c->ent_cf.
  PjFront(int32_t n, bool render_it, int16_t* cf_ext = nullptr)
      : info((size_t)(n > 0 ? n : 0)), render_it(render_it), cf_ext(cf_ext) {}
  int parse(int i, const uint8_t* data, int64_t len, jds_jpeg_info* frame) override {
    const int rc = pj_parse_file(data, len, &info[(size_t)i]);
    *frame = info[(size_t)i].frame;
    return rc;
  }
  int check(int i, const jds_jpeg_info*) override {
    if (render_it && !info[(size_t)i].complete)
      return fail(JDS_ENOTSUP, "incomplete progression: the scans do not code every coefficient down to Al = 0");
    return JDS_OK;
  }
  int describe(BatchJob& j) override {
    const BatchPlan& bp = j.bp;
    const int nv = (int)bp.recs.size();
    mcus.resize((size_t)nv);
    for (int k = 0; k < nv; ++k) {
      const int i = bp.file_of[(size_t)k];
      HdMcu m = hd_jpeg_mcu(&bp.info[(size_t)i]);
      for (int cc = 0; cc < 3; ++cc) m.off[cc] += bp.recs[(size_t)k].coef_off;
      mcus[(size_t)k] = m;
      if (!pj_build_chains(j.data[i], &info[(size_t)i], k, (long long)j.foff[(size_t)k], chains, scans, tabs))
        return fail(JDS_EINVAL, "file %d: DHT: BITS over-subscribe the code space", i);  // (the parser has refused these)
    }
    if (chains.size() > 0x7fffffffull || scans.size() > 0x7fffffffull || tabs.size() > 0x7fffffffull)
      return fail(JDS_ENOTSUP, "batch too long for one decode");
    o_tabs = j.add(tabs);
    o_mcu = j.add(mcus);
    o_scan = j.add(scans);
    o_chain = j.add(chains);
    if (!cf_ext) HIP_TRY(j.c->ent_cf.ensure(sizeof(int16_t) * (size_t)bp.coef_entries));
    j.cf_d = cf_ext ? cf_ext : (int16_t*)j.c->ent_cf.p;
    j.zero_p = j.cf_d;  // (progressive decoding accumulates)
    j.zero_n = sizeof(int16_t) * (size_t)bp.coef_entries;
    return JDS_OK;
  }
  int decode(BatchJob& j) override {
    ticks_d = nullptr;
    if (j.c->prof_on) {  // the walk time of every scan, for jds_pjpeg_scan_times
      HIP_TRY(j.c->pj_ticks.ensure(8 * scans.size()));
      ticks_d = (unsigned long long*)j.c->pj_ticks.p;
      HIP_TRY(hipMemsetAsync(ticks_d, 0, 8 * scans.size(), j.s));
    }
    HIP_TRY(launch_pjpeg_chains(j.dev<uint8_t>(0), j.files_bytes, j.dev<PjChain>(o_chain), (int)chains.size(),
                                j.dev<PjScan>(o_scan), j.dev<HuffDecTab>(o_tabs), j.dev<HdMcu>(o_mcu), j.cf_d, j.st_d,
                                ticks_d, j.s));
    return JDS_OK;
  }
  bool render_it;
  int16_t* cf_ext;
  std::vector<PjChain> chains;
  std::vector<HuffDecTab> tabs;
  std::vector<HdMcu> mcus;
  size_t o_tabs = 0, o_mcu = 0, o_scan = 0, o_chain = 0;
};

// batch_run (jds_abi_jpeg.hip) over progressive files, then the scans' walk times into the context.
static int pj_run(jds_ctx* c, BatchPlan& bp, PjFront& fe, const uint8_t* const* data, const int64_t* lens, uint8_t* rgb,
                  int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items, bool inverse, int32_t render) {
  const int rc = batch_run(c, bp, fe, data, lens, rgb, rgb_on_device, coeffs, items, inverse, render);
  if (rc) return rc;
  c->pj_scan_us.clear();
  if (!fe.ticks_d) return JDS_OK;
  std::vector<unsigned long long> t(fe.scans.size());
  int khz = 0;
  HIP_TRY(hipMemcpy(t.data(), fe.ticks_d, 8 * t.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
  for (unsigned long long v : t) c->pj_scan_us.push_back(khz > 0 ? (double)v * 1e3 / khz : 0.0);
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
  BatchPlan bp;
  PjFront fe(n, true);
  const int rc = batch_layout(data, lens, n, items, bp, fe, JDS_RENDER_LIBJPEG, scale_denoms, scaled);
  if (rc) return rc;
  *rgb_bytes = bp.rgb_bytes;
  *coef_entries = bp.coef_entries;
  batch_note(bp);
  return JDS_OK;
}

int jds_pjpeg_batch_to_rgb(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                           int64_t rgb_cap, int32_t rgb_on_device, int32_t render, const int32_t* scale_denoms,
                           jds_jpeg_batch_item* items, jds_jpeg_scaled_item* scaled, int16_t* coeffs) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!c) return fail(JDS_EINVAL, "null argument");
  BatchPlan bp;
  PjFront fe(n, true);
  if ((rc = batch_layout(data, lens, n, items, bp, fe, render, scale_denoms, scaled))) return rc;
  if (bp.rgb_bytes > 0 && (!rgb || rgb_cap < bp.rgb_bytes))
    return fail(JDS_EINVAL, "image buffer too small: %lld bytes needed", (long long)bp.rgb_bytes);
  if (!bp.recs.empty() && (rc = pj_run(c, bp, fe, data, lens, rgb, rgb_on_device, coeffs, items, true, render))) return rc;
  batch_note(bp);
  return JDS_OK;
}

static int pj_decode(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap, bool on_device,
                     jds_pjpeg_info* info) {
  if (!c || !data || !info) return fail(JDS_EINVAL, "null argument");
  BatchPlan bp;
  PjFront fe(1, false, on_device ? coeffs : nullptr);
  jds_jpeg_batch_item it;
  int rc;
  if ((rc = batch_layout(&data, &len, 1, &it, bp, fe))) return rc;
  *info = fe.info[0];
  batch_note(bp);
  if (it.rc == JDS_OK) {
    if ((rc = check_coef_cap(coeffs, coeffs_cap, info->frame.coeffs_needed))) return rc;
    if ((rc = pj_run(c, bp, fe, &data, &len, nullptr, 0, on_device ? nullptr : coeffs, &it, false, JDS_RENDER_REFERENCE)))
      return rc;
  }
  return pj_single_result(it.rc, it.status, info);
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
  BatchPlan bp;
  PjFront fe(1, true);
  jds_jpeg_batch_item it;
  if ((rc = batch_layout(&data, &len, 1, &it, bp, fe, render, &scale_denom))) return rc;
  *info = fe.info[0];
  batch_note(bp);
  if (it.rc == JDS_OK) {
    long long oh, ow;
    ls_scaled_size(it.H, it.W, scale_denom, &oh, &ow);
    if (rgb_cap < oh * ow * 3) return fail(JDS_EINVAL, "image buffer too small: %lld bytes needed", oh * ow * 3);
    if ((rc = pj_run(c, bp, fe, &data, &len, rgb_out, rgb_on_device, coeffs, &it, true, render))) return rc;
  }
  return pj_single_result(it.rc, it.status, info);
}

// The prefix of a transcoded progressive file: mcu_splice's (every segment before the first SOS
// except DHT and DRI), its SOF2 marker rewritten as SOF0.
static int pj_prefix(const uint8_t* data, int64_t len, McuJob* j) {
  const int rc = mcu_job_splice(data, len, j);
  if (rc) return rc;
  const int64_t n = (int64_t)j->pfx.size();
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
  BatchPlan bp;
  PjFront fe(n, false);
  int rc = batch_layout(data, lens, n, bi.data(), bp, fe);
  if (rc) return rc;
  if (!bp.recs.empty() && (rc = pj_run(c, bp, fe, data, lens, nullptr, 0, nullptr, bi.data(), false, JDS_RENDER_REFERENCE)))
    return rc;
  return batch_transcode_tail(
      c, bp, bi, n,
      [&](size_t k, int i, McuJob* j) {
        const int r = mcu_job_geo(&bp.info[(size_t)i], bp.recs[k].coef_off, j);
        return r ? r : pj_prefix(data[i], lens[i], j);
      },
      nullptr, optimize, out, out_cap, out_on_device, items, out_bytes);
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
  return pj_single_result(it.rc, it.status, info);
}

}  // extern "C"
