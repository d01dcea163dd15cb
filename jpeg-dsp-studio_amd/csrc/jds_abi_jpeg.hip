// jds_abi_jpeg.hip — the C-ABI's foreign-file half (include/jds.h): parse and
// decode of files of either scan form, rendering, batches, the lossless
// transcode and transforms, the libjpeg encoding, and their host models
// (jds_selftest_*).
//
// Host side only: descriptors (jds_dec_jobs.hpp), uploads and launches.
#include <algorithm>
#include <functional>
#include <string>

#include "jds_abi.hpp"
#include "jds_abi_jpeg.hpp"
#include "jds_dec_jobs.hpp"
#include "jds_entropy_mcu_dev.hpp"
#include "jds_jpeg_fwd.hpp"
#include "jds_jpeg_ljs.hpp"
#include "jds_jpeg_ljt.hpp"
#include "jds_jpeg_parse.hpp"
#include "jds_xform_dev.hpp"

extern "C" {

// ------------------------------------------------------ entropy decoding --

// Parse under a profile (jds_jpeg_parse.hpp: HD_OWN is jds_jfif_parse's, HD_ANY
// jds_jpeg_parse's), then the size the buffers' index arithmetic is made for.
static int parse_file(const uint8_t* data, int64_t len, HdProfile prof, jds_jpeg_info* out) {
  const int rc = hd_walk(data, len, prof, out, g_err, sizeof g_err);
  if (rc) return rc;
  if (out->H * out->W > (int64_t)1 << 28)
    return fail(JDS_EINVAL, "unsupported image size %lldx%lld", (long long)out->H, (long long)out->W);
  return JDS_OK;
}

int jds_jpeg_parse(const uint8_t* data, int64_t len, jds_jpeg_info* out) { return parse_file(data, len, HD_ANY, out); }

// The _jfif calls: the file parses under the own profile, the work runs on the
// general info (the bodies of the _jpeg calls below), and the caller's struct
// is that info's view (jfif_info_of), status and rounds included.
int jds_jfif_parse(const uint8_t* data, int64_t len, jds_jfif_info* out) {
  if (!out) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info j;
  const int rc = parse_file(data, len, HD_OWN, &j);
  memset(out, 0, sizeof *out);
  if (rc == JDS_OK) jfif_info_of(&j, out);
  return rc;
}

int check_coef_cap(const int16_t* coeffs, int64_t cap, int64_t needed) {
  if (!coeffs || cap < needed)
    return fail(JDS_EINVAL, "coefficient buffer too small: %lld entries needed", (long long)needed);
  return JDS_OK;
}

int jds_entropy_decode_info(int32_t* subseq_bits, int32_t* subseq_per_group) {
  if (!subseq_bits || !subseq_per_group) return fail(JDS_EINVAL, "null argument");
  int s, g;
  dec_constants(&s, &g);
  *subseq_bits = s;
  *subseq_per_group = g;
  return JDS_OK;
}

static int selftest_args(const int16_t* coeffs, const int32_t* rounds_out, int32_t subseq_bits) {
  if (!coeffs || !rounds_out) return fail(JDS_EINVAL, "null argument");
  if (subseq_bits < 64 || subseq_bits % 8) return fail(JDS_EINVAL, "subseq_bits must be a multiple of 8, at least 64");
  return JDS_OK;
}

// A parsed file through the host model; rounds[3]: per scan in file order.
static int host_decode_parsed(const uint8_t* data, const jds_jpeg_info* info, int32_t subseq_bits, int16_t* coeffs,
                              int64_t coeffs_cap, int32_t* rounds) {
  const int rc = check_coef_cap(coeffs, coeffs_cap, info->coeffs_needed);
  if (rc) return rc;
  int lane_max;
  rst_constants(&lane_max);
  const uint32_t st = hd_jpeg_host_decode(data, info, subseq_bits, lane_max, coeffs, rounds);
  if (st) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(st), st);
  return JDS_OK;
}

int jds_selftest_jpegdec(const uint8_t* data, int64_t len, int32_t subseq_bits, int16_t* coeffs, int64_t coeffs_cap,
                         int32_t* rounds_out) {
  jds_jpeg_info info;
  int rc;
  if ((rc = selftest_args(coeffs, rounds_out, subseq_bits)) || (rc = parse_file(data, len, HD_ANY, &info))) return rc;
  return host_decode_parsed(data, &info, subseq_bits, coeffs, coeffs_cap, rounds_out);
}

// rounds_out: per component (Y, Cb, Cr); an own-profile file may carry its scans in any order.
int jds_selftest_huffdec(const uint8_t* data, int64_t len, int32_t subseq_bits, int16_t* coeffs, int64_t coeffs_cap,
                         int32_t* rounds_out) {
  jds_jpeg_info info;
  int rc;
  if ((rc = selftest_args(coeffs, rounds_out, subseq_bits)) || (rc = parse_file(data, len, HD_OWN, &info))) return rc;
  int32_t rounds[3] = {0, 0, 0};
  rc = host_decode_parsed(data, &info, subseq_bits, coeffs, coeffs_cap, rounds);
  for (int i = 0; i < 3; ++i) rounds_out[info.scan[i].component[0] - 1] = rounds[i];
  return rc;
}

// A file's four decode tables ([0] DC 0, [1] DC 1, [2] AC 0, [3] AC 1; an
// undefined one stays zeroed).  False: a DHT's BITS over-subscribe the code space.
static bool dec_tables(const jds_jfif_huff* huff, HuffDecTab* tabs) {
  bool ok = true;
  for (int i = 0; i < 4; ++i) {
    memset(&tabs[i], 0, sizeof tabs[i]);
    if (huff[i].defined && hd_build(huff[i].bits, huff[i].vals, &tabs[i]) < 0) ok = false;
  }
  return ok;
}
static const char* const DHT_OVERSUBSCRIBED = "DHT: BITS over-subscribe the code space";

// A parsed file of either profile and scan form into c->ent_cf: the batch of
// one (defined behind batch_run).  Fills info->status and info->rounds.
static int decode_one(jds_ctx* c, const uint8_t* data, int64_t len, jds_jpeg_info* info);

// jds_decode_jpeg / _jfif once the file is parsed.
static int decode_parsed(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                         jds_jpeg_info* info) {
  int rc;
  if ((rc = check_coef_cap(coeffs, coeffs_cap, info->coeffs_needed))) return rc;
  if ((rc = decode_one(c, data, len, info))) return rc;
  HIP_TRY(hipMemcpy(coeffs, c->ent_cf.p, (size_t)info->coeffs_needed * sizeof(int16_t), hipMemcpyDeviceToHost));
  return JDS_OK;
}

int jds_decode_jpeg(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                    jds_jpeg_info* info) {
  if (!c || !data || !info) return fail(JDS_EINVAL, "null argument");
  const int rc = parse_file(data, len, HD_ANY, info);
  return rc ? rc : decode_parsed(c, data, len, coeffs, coeffs_cap, info);
}

int jds_decode_jfif(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                    jds_jfif_info* info) {
  if (!c || !data || !info) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info j;
  int rc = parse_file(data, len, HD_OWN, &j);
  if (rc) return rc;
  rc = decode_parsed(c, data, len, coeffs, coeffs_cap, &j);
  jfif_info_of(&j, info);  // (also where the coefficient buffer is too small)
  return rc;
}

// The parameter block of the plan's inverse for a file of 8x8 blocks with one quantisation table.
static jds_params params_of_file(int32_t subsampling, const double* qtable) {
  jds_params prm;
  memset(&prm, 0, sizeof prm);
  prm.block_size = 8;
  prm.quality = 0;
  prm.subsampling = subsampling;
  memcpy(prm.qtable, qtable, sizeof prm.qtable);
  return prm;
}

// jds_decompress_jpeg / _jfif once the file is parsed (an own-profile file passes the first two checks).
static int decompress_parsed(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                             int16_t* coeffs, jds_jpeg_info* info) {
  if (info->subsampling == JDS_SS_GRAY)
    return fail(JDS_ENOTSUP, "the plan's inverse takes three components: this is a grayscale file "
                             "(jds_jpeg_to_rgb reconstructs it)");
  if (!info->single_table || !info->reference_grid)
    return fail(JDS_ENOTSUP, "the plan's inverse takes one quantisation table and the reference's block grids: "
                             "%s (the per-stage calls reconstruct such a file)",
                info->single_table ? "this size has other grids" : "the file has a table per component");
  const size_t nimg = (size_t)info->H * (size_t)info->W * 3;
  if (rgb_cap < (int64_t)nimg) return fail(JDS_EINVAL, "image buffer too small: %zu bytes needed", nimg);
  const jds_params prm = params_of_file(info->subsampling, info->qtable[0]);
  int rc;
  if ((rc = check_tables(&prm))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = decode_one(c, data, len, info))) return rc;
  return inverse_of_decoded(c, &prm, info->H, info->W, info->coeffs_needed, rgb_out, coeffs);
}

int jds_decompress_jpeg(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                        int16_t* coeffs, jds_jpeg_info* info) {
  if (!c || !data || !info || !rgb_out) return fail(JDS_EINVAL, "null argument");
  const int rc = parse_file(data, len, HD_ANY, info);
  return rc ? rc : decompress_parsed(c, data, len, rgb_out, rgb_cap, coeffs, info);
}

int jds_decompress_jfif(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                        int16_t* coeffs, jds_jfif_info* info) {
  if (!c || !data || !info || !rgb_out) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info j;
  int rc = parse_file(data, len, HD_OWN, &j);
  if (rc) return rc;
  rc = decompress_parsed(c, data, len, rgb_out, rgb_cap, coeffs, &j);
  jfif_info_of(&j, info);
  return rc;
}

// ----------------------------------- foreign files to pixels (k_jpeg_inv) --

int jds_jpeg_inverse_info(int32_t* tile_h, int32_t* tile_w) {
  if (!tile_h || !tile_w) return fail(JDS_EINVAL, "null argument");
  int th, tw;
  jpeg_inv_constants(&th, &tw);
  *tile_h = th;
  *tile_w = tw;
  return JDS_OK;
}

// The rendering a _render call names: JDS_RENDER_REFERENCE (k_jpeg_inv) or
// JDS_RENDER_LIBJPEG (k_jpeg_ljt); anything else is the caller's error.
int render_check(int32_t render) {
  if (render != JDS_RENDER_REFERENCE && render != JDS_RENDER_LIBJPEG)
    return fail(JDS_EINVAL, "unknown render %d (JDS_RENDER_REFERENCE or JDS_RENDER_LIBJPEG)", (int)render);
  return JDS_OK;
}

// The denominator a _scaled call names: 1, 2, 4 or 8, and only the libjpeg
// rendering scales.
int scale_check(int32_t render, int32_t denom) {
  if (!ls_denom_ok(denom)) return fail(JDS_EINVAL, "scale_denom %d is not 1, 2, 4 or 8", (int)denom);
  if (denom != 1 && render != JDS_RENDER_LIBJPEG)
    return fail(JDS_EINVAL, "scale_denom %d needs JDS_RENDER_LIBJPEG: the reference rendering has no scaled decode",
                (int)denom);
  return JDS_OK;
}

// The launch arguments of a parsed file: its tables by check_tables' rule, its
// grids T.81's for H x W, every tile's chroma window within the kernel's arrays.
int jpeg_inv_args(const jds_jpeg_info* info, JInvArgs* a) {
  const int rc = jinv_args(info, a);
  if (rc == -1000)
    return fail(JDS_EINVAL, "jpeg inverse: %lldx%lld with these grids is not a T.81 geometry of subsampling %d",
                (long long)info->H, (long long)info->W, info->subsampling);
  if (rc < 0) {
    const int c = (-rc - 1) / 64, i = (-rc - 1) % 64;
    return fail(JDS_EINVAL, "qtable[%d][%d] = %g is not an integer in [1, 255]", c, i, info->qtable[c][i]);
  }
  if (!jpeg_inv_fits(*a))
    return fail(JDS_ENOTSUP, "jpeg inverse: a tile of %lldx%lld reads a wider chroma window than the kernel keeps",
                (long long)info->H, (long long)info->W);
  return JDS_OK;
}

static hipError_t launch_render(int32_t render, const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  return render == JDS_RENDER_LIBJPEG ? launch_jpeg_ljt(a, coeffs, rgb, s) : launch_jpeg_inv(a, coeffs, rgb, s);
}

int jds_jpeg_render_dev(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb, void* stream,
                        int32_t render) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!info) return fail(JDS_EINVAL, "null argument");
  JInvArgs a;
  if ((rc = jpeg_inv_args(info, &a))) return rc;
  if (!c || !coeffs || !rgb) return fail(JDS_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_render(render, a, coeffs, rgb, (hipStream_t)stream));
  return JDS_OK;
}

int jds_jpeg_scaled_size(int64_t H, int64_t W, int32_t scale_denom, int64_t* out_h, int64_t* out_w) {
  if (!out_h || !out_w) return fail(JDS_EINVAL, "null argument");
  if (!ls_denom_ok(scale_denom)) return fail(JDS_EINVAL, "scale_denom %d is not 1, 2, 4 or 8", (int)scale_denom);
  if (H < 1 || W < 1) return fail(JDS_EINVAL, "bad size %lldx%lld", (long long)H, (long long)W);
  long long oh, ow;
  ls_scaled_size(H, W, scale_denom, &oh, &ow);
  *out_h = oh;
  *out_w = ow;
  return JDS_OK;
}

int jds_jpeg_render_scaled_dev(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb, void* stream,
                               int32_t render, int32_t scale_denom) {
  int rc;
  if ((rc = render_check(render)) || (rc = scale_check(render, scale_denom))) return rc;
  if (scale_denom == 1) return jds_jpeg_render_dev(c, info, coeffs, rgb, stream, render);
  if (!info) return fail(JDS_EINVAL, "null argument");
  JInvArgs a;
  if ((rc = jpeg_inv_args(info, &a))) return rc;
  if (!c || !coeffs || !rgb) return fail(JDS_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_jpeg_ljs(a, scale_denom, coeffs, rgb, (hipStream_t)stream));
  return JDS_OK;
}

int jds_jpeg_inverse_dev(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb, void* stream) {
  return jds_jpeg_render_dev(c, info, coeffs, rgb, stream, JDS_RENDER_REFERENCE);
}

int jds_jpeg_to_rgb(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                    int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_info* info) {
  return jds_jpeg_to_rgb_render(c, data, len, rgb_out, rgb_cap, rgb_on_device, coeffs, info, JDS_RENDER_REFERENCE);
}

int jds_jpeg_to_rgb_render(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                           int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_info* info, int32_t render) {
  return jds_jpeg_to_rgb_scaled(c, data, len, rgb_out, rgb_cap, rgb_on_device, coeffs, info, render, 1);
}

int jds_jpeg_to_rgb_scaled(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                           int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_info* info, int32_t render,
                           int32_t scale_denom) {
  int rc;
  if ((rc = render_check(render)) || (rc = scale_check(render, scale_denom))) return rc;
  if (!c || !data || !info || !rgb_out) return fail(JDS_EINVAL, "null argument");
  rc = jds_jpeg_parse(data, len, info);
  if (rc) return rc;
  long long oh, ow;
  ls_scaled_size(info->H, info->W, scale_denom, &oh, &ow);
  const size_t nimg = (size_t)oh * (size_t)ow * 3;
  if (rgb_cap < (int64_t)nimg) return fail(JDS_EINVAL, "image buffer too small: %zu bytes needed", nimg);
  JInvArgs a;
  if ((rc = jpeg_inv_args(info, &a))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = decode_one(c, data, len, info))) return rc;  // (a defective scan: rgb_out is not written)
  uint8_t* dst = rgb_out;
  if (!rgb_on_device) {
    HIP_TRY(c->out.ensure(nimg));
    dst = (uint8_t*)c->out.p;
  }
  if (scale_denom == 1)
    HIP_TRY(launch_render(render, a, (const int16_t*)c->ent_cf.p, dst, c->stream));
  else
    HIP_TRY(launch_jpeg_ljs(a, scale_denom, (const int16_t*)c->ent_cf.p, dst, c->stream));
  if (!rgb_on_device) HIP_TRY(hipMemcpyAsync(rgb_out, dst, nimg, hipMemcpyDeviceToHost, c->stream));
  if (coeffs)
    HIP_TRY(hipMemcpyAsync(coeffs, c->ent_cf.p, (size_t)info->coeffs_needed * sizeof(int16_t), hipMemcpyDeviceToHost,
                           c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return JDS_OK;
}

int jds_selftest_jpeg_render(const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb_out, int32_t render) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!info || !coeffs || !rgb_out) return fail(JDS_EINVAL, "null argument");
  JInvArgs a;
  if ((rc = jpeg_inv_args(info, &a))) return rc;
  if (render == JDS_RENDER_LIBJPEG)
    jpeg_ljt_host_image(a, coeffs, rgb_out);
  else
    jpeg_inv_host(a, coeffs, rgb_out);
  return JDS_OK;
}

int jds_selftest_jpeg_render_scaled(const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb_out, int32_t render,
                                    int32_t scale_denom) {
  int rc;
  if ((rc = render_check(render)) || (rc = scale_check(render, scale_denom))) return rc;
  if (scale_denom == 1) return jds_selftest_jpeg_render(info, coeffs, rgb_out, render);
  if (!info || !coeffs || !rgb_out) return fail(JDS_EINVAL, "null argument");
  JInvArgs a;
  if ((rc = jpeg_inv_args(info, &a))) return rc;
  jpeg_ljs_host_image(a, scale_denom, coeffs, rgb_out);
  return JDS_OK;
}

int jds_selftest_jpeg_inverse(const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb_out) {
  return jds_selftest_jpeg_render(info, coeffs, rgb_out, JDS_RENDER_REFERENCE);
}

int jds_selftest_jpeg_window(int32_t d0, int32_t d1, int32_t dst_n, int32_t src_n, int32_t xaxis, int32_t* out) {
  if (!out || dst_n < 1 || src_n < 1 || d0 < 0 || d1 < d0 || d1 >= dst_n) return fail(JDS_EINVAL, "bad argument");
  jpeg_inv_window(d0, d1, 1.0 / ((double)dst_n / (double)src_n), src_n, xaxis != 0, &out[0], &out[1]);
  out[2] = JI_CAP_ROWS2;
  out[3] = JI_CAP_COLS2;
  return JDS_OK;
}

// ------------------------------------------- batches of foreign files --
// (DESIGN.md "Batches of foreign files")

// The baseline front end of the batch driver (jds_abi_jpeg.hpp): either scan
// form through the two decode groups and the restart-interval lanes.
struct BaselineFront : BatchFront {
  unsigned rounds = 0;  // the batch's propagation rounds, once it has run
  const char* too_long = "batch too long for one decode";  // (a single call names its scan)
  int parse(int, const uint8_t* data, int64_t len, jds_jpeg_info* frame) override {
    return jds_jpeg_parse(data, len, frame);
  }
  int check(int, const jds_jpeg_info* frame) override {
    HuffDecTab t[4];
    return dec_tables(frame->huff, t) ? JDS_OK : fail(JDS_EINVAL, "%s", DHT_OVERSUBSCRIBED);
  }
  // descriptors of both decode groups, lane intervals of both forms (a file's padded to whole workgroups)
  std::vector<DecScan> sc_il, sc_pl;
  std::vector<RstIv> iv_il, iv_pl;
  std::vector<HuffDecTab> tabs;
  std::vector<HdMcu> mcus;
  long long ng_il = 0, ng_pl = 0;
  int mx_il = 0, mx_pl = 0;
  size_t scr_il = 0, o_tabs = 0, o_mcu = 0, o_ivil = 0, o_ivpl = 0;
  int describe(BatchJob& j) override {
    jds_ctx* c = j.c;
    const BatchPlan& bp = j.bp;
    const int nv = (int)bp.recs.size();
    int lane_max;
    rst_constants(&lane_max);
    const int rst_g = rst_group_lanes();
    tabs.resize(4 * (size_t)nv);
    mcus.resize((size_t)nv);
    long long dcs_n = 0;
    for (int k = 0; k < nv; ++k) {
      const int i = bp.file_of[(size_t)k];
      const jds_jpeg_info& info = bp.info[(size_t)i];
      (void)dec_tables(info.huff, &tabs[4 * (size_t)k]);  // (the layout checked them)
      memset(&mcus[(size_t)k], 0, sizeof(HdMcu));
      const FilePlace pl{k, (long long)j.foff[(size_t)k], bp.recs[(size_t)k].coef_off, dcs_n};
      std::vector<DecScan>& sc = info.interleaved ? sc_il : sc_pl;
      std::vector<RstIv>& iv = info.interleaved ? iv_il : iv_pl;
      const size_t nsc0 = sc.size(), niv0 = iv.size();
      if (info.interleaved) {
        HdMcu m = hd_jpeg_mcu(&info);
        for (int cc = 0; cc < 3; ++cc) m.off[cc] += pl.coef_off;
        mcus[(size_t)k] = m;
        dcs_n += (long long)m.bpm * m.mcu_cols * m.mcu_rows;
      }
      const DecJobsResult jr = dec_jobs_build(j.data[i], dec_jobs_of(&info), pl, lane_max, sc, iv, g_err, sizeof g_err);
      if (jr == DEC_JOBS_MARKERS) {  // a defective scan, nothing of it is decoded
        sc.resize(nsc0);
        iv.resize(niv0);
        j.st0[(size_t)k] = HD_RESTART;
      } else if (jr) {
        return JDS_ENOTSUP;
      }
      while (iv.size() % (size_t)rst_g) {
        RstIv v{};
        v.file = v.frame = k;
        iv.push_back(v);
      }
    }
    if (sc_il.size() > 0x7fffffffull || sc_pl.size() > 0x7fffffffull || iv_il.size() > 0x7fffffffull ||
        iv_pl.size() > 0x7fffffffull)
      return fail(JDS_ENOTSUP, "too many restart intervals");
    ng_il = dec_layout(sc_il.data(), (int)sc_il.size(), &mx_il);
    ng_pl = dec_layout(sc_pl.data(), (int)sc_pl.size(), &mx_pl);
    if (ng_il < 0 || ng_pl < 0) return fail(JDS_ENOTSUP, "%s", too_long);
    o_tabs = j.add(tabs);
    o_mcu = j.add(mcus);
    o_ivil = j.add(iv_il);
    o_ivpl = j.add(iv_pl);
    scr_il = (dec_scratch_bytes(ng_il, (int)sc_il.size()) + 255) & ~(size_t)255;
    HIP_TRY(c->dec_scr.ensure(scr_il + dec_scratch_bytes(ng_pl, (int)sc_pl.size())));
    HIP_TRY(c->dec_mcu.ensure(sizeof(int16_t) * (size_t)dcs_n));
    HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)bp.coef_entries));
    j.cf_d = (int16_t*)c->ent_cf.p;
    j.zero_p = c->dec_mcu.p;  // the DC staging array of the interleaved scans
    j.zero_n = sizeof(int16_t) * (size_t)dcs_n;
    return JDS_OK;
  }

  int decode(BatchJob& j) override {
    jds_ctx* c = j.c;
    const uint8_t* files_d = j.dev<uint8_t>(0);
    const HuffDecTab* tabs_d = j.dev<HuffDecTab>(o_tabs);
    const HdMcu* mcu_d = j.dev<HdMcu>(o_mcu);
    const DecGroup grp[2] = {{sc_il.data(), (int)sc_il.size(), ng_il, mx_il, c->dec_scr.p, true},
                             {sc_pl.data(), (int)sc_pl.size(), ng_pl, mx_pl, (char*)c->dec_scr.p + scr_il, false}};
    int too_many = 0;
    HIP_TRY(dec_run_groups(files_d, grp, 2, tabs_d, j.cf_d, j.bp.coef_entries, j.st_d, j.s, &rounds, &too_many, mcu_d,
                           (int16_t*)c->dec_mcu.p));
    if (too_many)
      return fail(JDS_EHIP, "entropy decode: propagation did not settle within %d rounds", mx_il > mx_pl ? mx_il : mx_pl);
    HIP_TRY(launch_dec_rst(files_d, j.dev<RstIv>(o_ivil), (long long)iv_il.size(), tabs_d, j.cf_d, j.st_d, j.s, mcu_d));
    HIP_TRY(launch_dec_rst(files_d, j.dev<RstIv>(o_ivpl), (long long)iv_pl.size(), tabs_d, j.cf_d, j.st_d, j.s, nullptr));
    return JDS_OK;
  }
};

int batch_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items, BatchPlan& bp,
                 BatchFront& fe, int32_t render, const int32_t* denoms, jds_jpeg_scaled_item* scaled,
                 const int64_t* draft) {
  if (n < 0 || (n > 0 && (!data || !lens || !items))) return fail(JDS_EINVAL, "null argument");
  for (int i = 0; denoms && i < n; ++i) {
    if (!ls_denom_ok(denoms[i])) return fail(JDS_EINVAL, "file %d: scale_denom %d is not 1, 2, 4 or 8", i, (int)denoms[i]);
    const int rc = scale_check(render, denoms[i]);
    if (rc) return rc;
  }
  bp.info.resize((size_t)n);
  bp.rec_of.assign((size_t)n, -1);
  bp.denom.assign((size_t)n, 1);
  std::vector<JInvRec> parsed((size_t)n);
  std::vector<std::string> msg((size_t)n);  // (the message of a failing file: g_err is per thread)
  batch_parallel(n, [&](int i) {
    jds_jpeg_batch_item& it = items[i];
    memset(&it, 0, sizeof it);
    it.rgb_off = -1;
    it.coef_off = -1;
    jds_jpeg_info& info = bp.info[(size_t)i];
    JInvRec& r = parsed[(size_t)i];
    memset(&r, 0, sizeof r);
    int rc = data[i] && lens[i] >= 0 ? fe.parse(i, data[i], lens[i], &info) : fail(JDS_EINVAL, "null file");
    if (rc == JDS_OK) {
      it.H = info.H;
      it.W = info.W;
      it.subsampling = info.subsampling;
      it.interleaved = info.interleaved;
      rc = jpeg_inv_args(&info, &r.a);
    }
    if (rc == JDS_OK) rc = fe.check(i, &info);
    it.rc = rc;
    if (rc != JDS_OK) msg[(size_t)i] = g_err;
  });
  for (int i = 0; i < n; ++i) {
    jds_jpeg_batch_item& it = items[i];
    const jds_jpeg_info& info = bp.info[(size_t)i];
    JInvRec& r = parsed[(size_t)i];
    if (it.rc != JDS_OK) {
      bp.bad(i, msg[(size_t)i].c_str());
      continue;
    }
    long long rb = bp.rgb_bytes, ce = bp.coef_entries;
    int dn = denoms ? denoms[i] : 1;
    if (!denoms && draft) {
      const int64_t sc = info.W / draft[0] < info.H / draft[1] ? info.W / draft[0] : info.H / draft[1];
      dn = sc >= 8 ? 8 : sc >= 4 ? 4 : sc >= 2 ? 2 : 1;
    }
    bp.denom[(size_t)i] = dn;
    ls_batch_place(r, (int)bp.recs.size(), dn, info.coeffs_needed, &rb, &ce);
    bp.any_scaled = bp.any_scaled || dn != 1;
    bp.rgb_bytes = rb;
    bp.coef_entries = ce;
    it.rgb_off = r.rgb_off;
    it.coef_off = r.coef_off;
    it.coeffs_needed = info.coeffs_needed;
    bp.rec_of[(size_t)i] = r.st;
    bp.file_of.push_back(i);
    bp.recs.push_back(r);
  }
  // what the grids and the 32-bit indices of the kernels take
  if (bp.coef_entries / 64 > 0x7fffffffll || !ls_batch_maps(bp.recs.data(), (int)bp.recs.size(), bp.map, bp.smap))
    return fail(JDS_ENOTSUP, "batch of %d files: too many blocks or tiles for one set of launches", n);
  for (int i = 0; scaled && i < n; ++i) {
    memset(&scaled[i], 0, sizeof scaled[i]);
    scaled[i].scale_denom = denoms ? denoms[i] : bp.denom[(size_t)i];
    if (items[i].rc != JDS_OK) continue;
    long long oh, ow;
    ls_scaled_size(items[i].H, items[i].W, scaled[i].scale_denom, &oh, &ow);
    scaled[i].out_h = oh;
    scaled[i].out_w = ow;
  }
  return JDS_OK;
}

void batch_note(const BatchBad& b, const char* what) {
  if (b.first_bad >= 0) {
    char m[400];
    snprintf(m, sizeof m, "%s", b.first_msg);
    fail(0, "%s %d: %s", what, b.first_bad, m);
  } else {
    g_err[0] = 0;
  }
}

int jds_jpeg_batch_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items,
                          int64_t* rgb_bytes, int64_t* coef_entries) {
  return jds_jpeg_batch_layout_scaled(data, lens, n, items, rgb_bytes, coef_entries, nullptr, nullptr);
}

int jds_jpeg_batch_layout_scaled(const uint8_t* const* data, const int64_t* lens, int32_t n,
                                 jds_jpeg_batch_item* items, int64_t* rgb_bytes, int64_t* coef_entries,
                                 const int32_t* scale_denoms, jds_jpeg_scaled_item* scaled) {
  if (!rgb_bytes || !coef_entries) return fail(JDS_EINVAL, "null argument");
  BatchPlan bp;
  BaselineFront fe;
  const int rc = batch_layout(data, lens, n, items, bp, fe, JDS_RENDER_LIBJPEG, scale_denoms, scaled);
  if (rc) return rc;
  *rgb_bytes = bp.rgb_bytes;
  *coef_entries = bp.coef_entries;
  batch_note(bp);
  return JDS_OK;
}

int jds_selftest_jpeg_batch(const uint8_t* const* data, const int64_t* lens, int32_t n, int32_t subseq_bits,
                            uint8_t* rgb, int64_t rgb_cap, int16_t* coeffs, jds_jpeg_batch_item* items) {
  return jds_selftest_jpeg_batch_render(data, lens, n, subseq_bits, rgb, rgb_cap, coeffs, items, JDS_RENDER_REFERENCE);
}

int jds_selftest_jpeg_batch_render(const uint8_t* const* data, const int64_t* lens, int32_t n, int32_t subseq_bits,
                                   uint8_t* rgb, int64_t rgb_cap, int16_t* coeffs, jds_jpeg_batch_item* items,
                                   int32_t render) {
  return jds_selftest_jpeg_batch_render_scaled(data, lens, n, subseq_bits, rgb, rgb_cap, coeffs, items, render, nullptr,
                                               nullptr);
}

int jds_selftest_jpeg_batch_render_scaled(const uint8_t* const* data, const int64_t* lens, int32_t n,
                                          int32_t subseq_bits, uint8_t* rgb, int64_t rgb_cap, int16_t* coeffs,
                                          jds_jpeg_batch_item* items, int32_t render, const int32_t* scale_denoms,
                                          jds_jpeg_scaled_item* scaled) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (subseq_bits < 64 || subseq_bits % 8) return fail(JDS_EINVAL, "subseq_bits must be a multiple of 8, at least 64");
  BatchPlan bp;
  BaselineFront fe;
  rc = batch_layout(data, lens, n, items, bp, fe, render, scale_denoms, scaled);
  if (rc) return rc;
  if (bp.rgb_bytes > 0 && (!rgb || rgb_cap < bp.rgb_bytes))
    return fail(JDS_EINVAL, "image buffer too small: %lld bytes needed", (long long)bp.rgb_bytes);
  std::vector<int16_t> own;
  if (!coeffs) {
    own.resize((size_t)bp.coef_entries);
    coeffs = own.data();
  }
  int lane_max;
  rst_constants(&lane_max);
  std::vector<uint32_t> st(bp.recs.size() + 1, 0u);
  for (size_t k = 0; k < bp.recs.size(); ++k) {
    const int i = bp.file_of[k];
    int32_t rounds[3];
    st[k] = hd_jpeg_host_decode(data[i], &bp.info[(size_t)i], subseq_bits, lane_max, coeffs + bp.recs[k].coef_off, rounds);
    items[i].status = st[k];
  }
  const JInvMap* maps[JI_MODES];
  int nmap[JI_MODES];
  for (int m = 0; m < JI_MODES; ++m) {
    maps[m] = bp.map[m].data();
    nmap[m] = (int)bp.map[m].size() - 1;
  }
  if (render == JDS_RENDER_LIBJPEG)
    jpeg_ljt_batch_host(bp.recs.data(), maps, nmap, st.data(), coeffs, rgb);
  else
    jpeg_inv_batch_host(bp.recs.data(), maps, nmap, st.data(), coeffs, rgb);
  if (bp.any_scaled) {  // (scale_check: the libjpeg rendering)
    const JInvMap* smaps[JI_MODES][LS_ND];
    int nsmap[JI_MODES][LS_ND];
    for (int m = 0; m < JI_MODES; ++m)
      for (int d = 0; d < LS_ND; ++d) {
        smaps[m][d] = bp.smap[m][d].data();
        nsmap[m][d] = (int)bp.smap[m][d].size() - 1;
      }
    jpeg_ljs_batch_host(bp.recs.data(), smaps, nsmap, st.data(), coeffs, rgb);
  }
  batch_note(bp);
  return JDS_OK;
}

int batch_run(jds_ctx* c, BatchPlan& bp, BatchFront& fe, const uint8_t* const* data, const int64_t* lens, uint8_t* rgb,
              int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items, bool inverse, int32_t render,
              const std::function<int(const uint32_t*, hipStream_t)>* after) {
  const int nv = (int)bp.recs.size();
  hipStream_t s = c->stream;
  HIP_TRY(hipSetDevice(c->device));
  BatchJob j{c, s, bp, data};
  // the upload: the files (at 16-byte boundaries inside their section), the decode's descriptors,
  // the inverse records, the tile maps of every launch, the status words
  j.foff.resize((size_t)nv);
  size_t o = 0;
  for (int k = 0; k < nv; ++k) {
    j.foff[(size_t)k] = o;
    o = (o + (size_t)lens[bp.file_of[(size_t)k]] + 15) / 16 * 16;
  }
  j.add(nullptr, o);  // (at 0)
  j.files_bytes = (long long)j.total;
  j.st0.assign((size_t)nv, 0u);
  int rc;
  if ((rc = fe.describe(j))) return rc;
  std::vector<JInvMap> maps;
  int map_off[JI_MODES], nmap[JI_MODES], tiles[JI_MODES];
  for (int m = 0; m < JI_MODES; ++m) {
    map_off[m] = (int)maps.size();
    nmap[m] = (int)bp.map[m].size() - 1;
    tiles[m] = bp.map[m].back().tile0;
    maps.insert(maps.end(), bp.map[m].begin(), bp.map[m].end());
  }
  int smap_off[JI_MODES][LS_ND], nsmap[JI_MODES][LS_ND], stiles[JI_MODES][LS_ND];
  for (int m = 0; m < JI_MODES; ++m)
    for (int d = 0; d < LS_ND; ++d) {  // (a batch without scaled images uploads what it always did)
      smap_off[m][d] = (int)maps.size();
      nsmap[m][d] = bp.any_scaled ? (int)bp.smap[m][d].size() - 1 : 0;
      stiles[m][d] = bp.any_scaled ? bp.smap[m][d].back().tile0 : 0;
      if (bp.any_scaled) maps.insert(maps.end(), bp.smap[m][d].begin(), bp.smap[m][d].end());
    }
  const size_t o_rec = j.add(bp.recs), o_map = j.add(maps), o_st = j.add(j.st0);
  if (j.total > c->bat_host_cap) {  // the staging buffer and its device copy, grown to the upload's size
    if (c->bat_host) (void)hipHostFree(c->bat_host);
    c->bat_host = nullptr;
    c->bat_host_cap = 0;
    HIP_TRY(hipHostMalloc(&c->bat_host, j.total, hipHostMallocDefault));
    c->bat_host_cap = j.total;
  }
  HIP_TRY(c->bat.ensure(j.total));
  char* h = (char*)c->bat_host;
  for (const BatchJob::Part& p : j.parts)
    if (p.src && p.bytes) memcpy(h + p.off, p.src, p.bytes);
  batch_parallel(nv, [&](int k) {
    const int i = bp.file_of[(size_t)k];
    memcpy(h + j.foff[(size_t)k], data[i], (size_t)lens[i]);
  });
  uint8_t* dst = rgb;
  if (inverse && !rgb_on_device) {
    HIP_TRY(c->out.ensure((size_t)bp.rgb_bytes));
    dst = (uint8_t*)c->out.p;
  }
  j.dv = (char*)c->bat.p;
  j.st_d = (uint32_t*)(j.dv + o_st);
  const CtxMarkScope marks_(c, s);
  HIP_TRY(hipMemcpyAsync(j.dv, h, j.total, hipMemcpyHostToDevice, s));
  if (j.zero_n) HIP_TRY(hipMemsetAsync(j.zero_p, 0, j.zero_n, s));
  kmark(s, "(batch upload)");
  if ((rc = fe.decode(j))) return rc;
  const JInvRec* rec_d = j.dev<JInvRec>(o_rec);
  const JInvMap* map_d = j.dev<JInvMap>(o_map);
  if (inverse && render == JDS_RENDER_LIBJPEG)
    HIP_TRY(launch_jpeg_ljt_batch(rec_d, map_d, map_off, nmap, tiles, j.st_d, j.cf_d, dst, s));
  else if (inverse)
    HIP_TRY(launch_jpeg_inv_batch(rec_d, map_d, map_off, nmap, tiles, j.st_d, j.cf_d, dst, s));
  if (inverse && bp.any_scaled)
    HIP_TRY(launch_jpeg_ljs_batch(rec_d, map_d, smap_off, nsmap, stiles, j.st_d, j.cf_d, dst, s));
  if (after) {  // (jds_jpeg_batch_to_tensor: the resize behind the rendering, on the same stream)
    if ((rc = (*after)(j.st_d, s))) return rc;
  }
  if (inverse && !rgb_on_device)  // image by image: the gaps of the caller's buffer stay as they are
    for (int k = 0; k < nv; ++k) {
      const JInvRec& r = bp.recs[(size_t)k];
      long long oh, ow;
      ls_scaled_size(r.a.H, r.a.W, ls_rec_denom(r), &oh, &ow);
      HIP_TRY(hipMemcpyAsync(rgb + r.rgb_off, dst + r.rgb_off, (size_t)oh * (size_t)ow * 3, hipMemcpyDeviceToHost, s));
    }
  if (coeffs)
    HIP_TRY(hipMemcpyAsync(coeffs, j.cf_d, sizeof(int16_t) * (size_t)bp.coef_entries, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(j.st0.data(), j.st_d, 4 * (size_t)nv, hipMemcpyDeviceToHost, s));
  kmark(s, "(batch download)");
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < nv; ++k) items[bp.file_of[(size_t)k]].status = j.st0[(size_t)k];
  return JDS_OK;
}

int single_result(int item_rc, uint32_t status) {
  if (item_rc) {
    std::string m = g_err;
    if (m.rfind("file 0: ", 0) == 0) m = m.substr(8);
    return fail(item_rc, "%s", m.c_str());
  }
  if (status) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(status), status);
  return JDS_OK;
}

// The one way a single baseline file reaches the device: the plan of its frame
// (no second parse, none of the renderings' checks) through batch_run without
// the inverse; the single-image renderings and the writer follow in the callers.
// The front end's HD_RESTART for DEC_JOBS_MARKERS is never this call's result:
// the parser that filled *info counted in each scan exactly the RSTm markers
// next_rst finds, one fewer than its intervals, so the builder finds them all.
static int decode_one(jds_ctx* c, const uint8_t* data, int64_t len, jds_jpeg_info* info) {
  BaselineFront fe;
  fe.too_long = "scan too long";
  int rc;
  if ((rc = fe.check(0, info))) return rc;  // (before anything is uploaded)
  BatchPlan bp(*info);
  jds_jpeg_batch_item it;  // (its status is all a run writes)
  if ((rc = batch_run(c, bp, fe, &data, &len, nullptr, 0, nullptr, &it, false))) return rc;
  info->status = it.status;
  info->rounds = fe.rounds;
  return single_result(JDS_OK, it.status);
}

int jds_jpeg_batch_to_rgb(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                          int64_t rgb_cap, int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items,
                          uint32_t* rounds_out) {
  return jds_jpeg_batch_to_rgb_render(c, data, lens, n, rgb, rgb_cap, rgb_on_device, coeffs, items, rounds_out,
                                      JDS_RENDER_REFERENCE);
}

int jds_jpeg_batch_to_rgb_render(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                                 int64_t rgb_cap, int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items,
                                 uint32_t* rounds_out, int32_t render) {
  return jds_jpeg_batch_to_rgb_scaled(c, data, lens, n, rgb, rgb_cap, rgb_on_device, coeffs, items, rounds_out, render,
                                      nullptr, nullptr);
}

int jds_jpeg_batch_to_rgb_scaled(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                                 int64_t rgb_cap, int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items,
                                 uint32_t* rounds_out, int32_t render, const int32_t* scale_denoms,
                                 jds_jpeg_scaled_item* scaled) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!c) return fail(JDS_EINVAL, "null argument");
  BatchPlan bp;
  BaselineFront fe;
  rc = batch_layout(data, lens, n, items, bp, fe, render, scale_denoms, scaled);
  if (rc) return rc;
  if (rounds_out) *rounds_out = 0;
  if (bp.rgb_bytes > 0 && (!rgb || rgb_cap < bp.rgb_bytes))
    return fail(JDS_EINVAL, "image buffer too small: %lld bytes needed", (long long)bp.rgb_bytes);
  if (!bp.recs.empty() && (rc = batch_run(c, bp, fe, data, lens, rgb, rgb_on_device, coeffs, items, true, render)))
    return rc;
  if (rounds_out) *rounds_out = fe.rounds;
  batch_note(bp);
  return JDS_OK;
}

// The decode above with JDS_RENDER_LIBJPEG into scratch of the context, then
// the batch resize behind it on the same stream (jds_abi_resize.hip; DESIGN.md
// "Pillow resizing").
int jds_jpeg_batch_to_tensor(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, int64_t out_h,
                             int64_t out_w, int32_t resample, const int32_t* scale_denoms, const float* boxes,
                             uint8_t* out, int64_t out_cap, int32_t out_on_device, jds_jpeg_batch_item* items,
                             jds_jpeg_scaled_item* scaled, uint32_t* rounds_out) {
  if (!c) return fail(JDS_EINVAL, "null argument");
  if (out_h < 1 || out_w < 1)
    return fail(JDS_EINVAL, "bad size: %lld x %lld (width x height)", (long long)out_w, (long long)out_h);
  if (out_h * out_w > 0x7fffffffll / 3 || out_h > 0x7fffffffll || out_w > 0x7fffffffll)
    return fail(JDS_ENOTSUP, "image too large: more than 2^31 - 1 bytes");
  const int64_t slot = out_h * out_w * 3, draft[2] = {out_w, out_h};
  BatchPlan bp;
  BaselineFront fe;
  int rc = batch_layout(data, lens, n, items, bp, fe, JDS_RENDER_LIBJPEG, scale_denoms, scaled, draft);
  if (rc) return rc;
  if (rounds_out) *rounds_out = 0;
  if (n > 0 && (!out || out_cap < slot * n))
    return fail(JDS_EINVAL, "output too small: %lld bytes needed", (long long)(slot * n));
  std::vector<ResizeSrc> src((size_t)n);
  for (int i = 0; i < n; ++i) {
    ResizeSrc& r = src[(size_t)i];
    memset(&r, 0, sizeof r);
    r.st = -1;
    r.zero = items[i].rc != JDS_OK;
    if (r.zero) continue;
    const JInvRec& rec = bp.recs[(size_t)bp.rec_of[(size_t)i]];
    long long oh, ow;
    ls_scaled_size(items[i].H, items[i].W, bp.denom[(size_t)i], &oh, &ow);
    r.off = rec.rgb_off;
    r.H = oh;
    r.W = ow;
    r.st = rec.st;
    r.has_box = boxes != nullptr;
    for (int k = 0; boxes && k < 4; ++k) r.box[k] = boxes[4 * (size_t)i + k];
  }
  ResizeJob* job = nullptr;
  if ((rc = resize_job_build(src.data(), n, out_h, out_w, resample, &job))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  uint8_t* dst = out;
  hipError_t e = c->rsz_src.ensure((size_t)bp.rgb_bytes);
  if (e == hipSuccess && !out_on_device && n > 0) {
    e = c->out.ensure((size_t)(slot * n));
    dst = (uint8_t*)c->out.p;
  }
  if (e != hipSuccess) {
    resize_job_free(job);
    HIP_TRY(e);
  }
  const std::function<int(const uint32_t*, hipStream_t)> after = [&](const uint32_t* st_d, hipStream_t s) -> int {
    const int r2 = resize_job_enqueue(c, job, (const uint8_t*)c->rsz_src.p, st_d, dst, s, false);
    if (r2) return r2;
    if (!out_on_device) HIP_TRY(hipMemcpyAsync(out, dst, (size_t)(slot * n), hipMemcpyDeviceToHost, s));
    return JDS_OK;
  };
  if (!bp.recs.empty()) {
    rc = batch_run(c, bp, fe, data, lens, (uint8_t*)c->rsz_src.p, 1, nullptr, items, true, JDS_RENDER_LIBJPEG, &after);
    if (rc == JDS_OK && rounds_out) *rounds_out = fe.rounds;
  } else if (n > 0) {  // no file decodes: every slot is zeros
    rc = after(nullptr, c->stream);
    if (rc == JDS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(JDS_EHIP, "hipStreamSynchronize");
  }
  resize_job_free(job);
  if (rc) return rc;
  batch_note(bp);
  return JDS_OK;
}

// ------------------------------------------------- lossless transcode --
// (DESIGN.md "Transcode"; kernels: jds_entropy_mcu.hip)

// One file of a writer batch: its geometry record (the planes' offsets count
// from the start of c->ent_cf) and its header prefix.
// (struct McuJob: jds_abi_jpeg.hpp, shared with jds_abi_pjpeg.hip)
int mcu_job_geo(const jds_jpeg_info* info, int64_t coef_off, McuJob* j) {
  if (mcu_file_of(info, &j->f))
    return fail(JDS_EINVAL,
                "%lldx%lld with block grids %lldx%lld, %lldx%lld, %lldx%lld is not a T.81 geometry of subsampling %d",
                (long long)info->H, (long long)info->W, (long long)info->grid_rows[0], (long long)info->grid_cols[0],
                (long long)info->grid_rows[1], (long long)info->grid_cols[1], (long long)info->grid_rows[2],
                (long long)info->grid_cols[2], info->subsampling);
  for (int cc = 0; cc < 3; ++cc) j->f.off[cc] += coef_off;
  return JDS_OK;
}

int mcu_job_splice(const uint8_t* data, int64_t len, McuJob* j) {
  const int64_t n = mcu_splice(data, len, nullptr, 0);
  if (n < 0 || n > 0x7fffffffll) return fail(JDS_EINVAL, "header splice: no marker sequence from SOI to an SOS");
  j->pfx.resize((size_t)n);
  if (mcu_splice(data, len, j->pfx.data(), n) != n) return fail(JDS_EINVAL, "header splice: length mismatch");
  return JDS_OK;
}

static int mcu_job_prefix(const jds_jpeg_info* info, const uint8_t* prefix, int64_t prefix_len, McuJob* j) {
  if (prefix) {
    if (prefix_len < 0 || prefix_len > 0x7fffffffll) return fail(JDS_EINVAL, "prefix_len %lld", (long long)prefix_len);
    j->pfx.assign(prefix, prefix + prefix_len);
    return JDS_OK;
  }
  j->pfx.resize(MCU_PFX_DEFAULT_MAX);
  const int n = mcu_default_prefix(info, j->pfx.data());
  if (n == -1000) return fail(JDS_EINVAL, "quantisation table id outside 0..3");
  if (n < 0) {
    const int cc = (-n - 1) / 64, i = (-n - 1) % 64;
    return fail(JDS_EINVAL, "qtable[%d][%d] = %g is not an integer in [1, 255]", cc, i, info->qtable[cc][i]);
  }
  j->pfx.resize((size_t)n);
  return JDS_OK;
}

static const char* const MCU_NOT_CODABLE =
    "not baseline-codable: a DC difference category above 11 or an AC category above 10";

// The Annex K table object on this thread's host side (and, with a context, on its device).
static int mcu_tables(jds_ctx* c, const char** host) {
  alignas(16) static thread_local char t[16384];
  static thread_local bool built = false;
  if (ent_tab_size() > sizeof t) return fail(JDS_EINVAL, "entropy tables exceed the staging buffer");
  if (!built) {
    ent_build_tables((EntTab*)t);
    built = true;
  }
  if (c && !c->ent_tab.p) {
    HIP_TRY(c->ent_tab.ensure(ent_tab_size()));
    HIP_TRY(hipMemcpy(c->ent_tab.p, t, ent_tab_size(), hipMemcpyHostToDevice));
  }
  *host = t;
  return JDS_OK;
}

static void mcu_std_tabs(McuStdTabs* t) {
  for (int i = 0; i < 4; ++i) t->n_vals[i] = ent_std_table(i, &t->bits[i], &t->vals[i]);
}

// The transformed files of a writer batch (DESIGN.md "Lossless transforms"):
// their records, tiles assigned, travel in the writer's upload and
// k_coef_xform runs in front of the writer's first kernel.
struct XfSet {
  std::vector<XfFile> files;
  int64_t tiles = 0;
  void add(XfFile f) {
    tiles += xf_set_tiles(&f, tiles);
    files.push_back(f);
  }
};

struct McuRun {
  McuDev d;
  int nf = 0, nseg = 0;
  std::vector<int64_t> len;  // per job: the file's bytes, 0: not baseline-codable
};

// The writer's launches up to the files' lengths, over the coefficients in
// c->ent_cf; the lengths and flags come back (the call's one read between the
// placement and the emit).
static int mcu_code(jds_ctx* c, std::vector<McuJob>& jobs, int optimize, McuRun* r, const XfSet* xf = nullptr) {
  hipStream_t s = c->stream;
  const int nf = (int)jobs.size();
  long long nseg = 0, raw_words = 0, pfx_bytes = 0;
  bool any_long = false;
  for (int k = 0; k < nf; ++k) {
    McuFile& f = jobs[(size_t)k].f;
    f.seg0 = (int32_t)nseg;
    f.frame = optimize ? k : 0;
    f.raw_w0 = raw_words;
    f.raw_words = mcu_raw_words(f.nblk);
    f.pfx_off = pfx_bytes;
    f.pfx_len = (int32_t)jobs[(size_t)k].pfx.size();
    if (f.gray) f.comp_id = mcu_gray_id(jobs[(size_t)k].pfx.data(), f.pfx_len);
    nseg += f.nseg;
    raw_words += f.raw_words;
    pfx_bytes += f.pfx_len;
    any_long = any_long || f.nseg > mcu_self_max();
    if (nseg > 0x1fffffffll || raw_words > 0x7fffffffll * 16)
      return fail(JDS_ENOTSUP, "batch of %d files: too many blocks for one set of writer launches", nf);
  }
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t nxf = xf ? xf->files.size() : 0, nxt = xf ? (size_t)xf->tiles : 0;
  if (nxt > 0x7fffffffull) return fail(JDS_ENOTSUP, "batch of %d files: too many blocks for one transform launch", nf);
  const size_t o_seg = up(sizeof(McuFile) * (size_t)nf), o_pfx = up(o_seg + 4 * (size_t)nseg),
               o_xf = up(o_pfx + (size_t)pfx_bytes), o_xt = nxf ? up(o_xf + sizeof(XfFile) * nxf) : o_xf,
               total = nxf ? up(o_xt + 4 * nxt) : o_xf;
  std::vector<char> h(total, 0);
  for (size_t k = 0; k < nxf; ++k) {
    const XfFile& x = xf->files[k];
    memcpy(h.data() + o_xf + sizeof(XfFile) * k, &x, sizeof(XfFile));
    int32_t* tf = (int32_t*)(h.data() + o_xt) + x.tile0;
    const int64_t nt = (k + 1 < nxf ? (int64_t)xf->files[k + 1].tile0 : xf->tiles) - x.tile0;
    for (int64_t i = 0; i < nt; ++i) tf[i] = (int32_t)k;
  }
  for (int k = 0; k < nf; ++k) {
    const McuJob& j = jobs[(size_t)k];
    memcpy(h.data() + sizeof(McuFile) * (size_t)k, &j.f, sizeof(McuFile));
    int32_t* sf = (int32_t*)(h.data() + o_seg) + j.f.seg0;
    for (int i = 0; i < j.f.nseg; ++i) sf[i] = k;
    if (!j.pfx.empty()) memcpy(h.data() + o_pfx + j.f.pfx_off, j.pfx.data(), j.pfx.size());
  }
  const char* tab_host;
  int rc = mcu_tables(c, &tab_host);
  if (rc) return rc;
  HIP_TRY(c->mcu_up.ensure(total));
  HIP_TRY(c->mcu_scr.ensure(mcu_scratch_bytes(nf, nseg, raw_words)));
  McuDev& d = r->d;
  (void)mcu_carve(c->mcu_scr.p, nf, nseg, raw_words, &d);
  d.files = (const McuFile*)c->mcu_up.p;
  d.segfile = (const int32_t*)((const char*)c->mcu_up.p + o_seg);
  d.pfx = (const uint8_t*)c->mcu_up.p + o_pfx;
  // a header template: the DHT segments a table class falls back to (its other bytes are not used)
  uint8_t hdr[ENT_HDR];
  double ones[64];
  for (double& v : ones) v = 1.0;
  if (ent_header(ones, M444, 8, 8, hdr) != ENT_HDR) return fail(JDS_EINVAL, "header template");
  std::vector<char> frame(mcu_optframe_bytes());
  mcu_std_frame(ent_es_tab(tab_host), hdr, frame.data());
  HIP_TRY(hipMemcpyAsync(c->mcu_up.p, h.data(), total, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d.hdr_std, hdr, ENT_HDR, hipMemcpyHostToDevice, s));
  if (!optimize) HIP_TRY(hipMemcpyAsync(d.of, frame.data(), frame.size(), hipMemcpyHostToDevice, s));
  if (nxf)  // the transformed files' planes into the second coefficient region, where their McuFile points
    HIP_TRY(launch_coef_xform((const XfFile*)((const char*)c->mcu_up.p + o_xf),
                              (const int32_t*)((const char*)c->mcu_up.p + o_xt), (long long)nxt,
                              (const int16_t*)c->ent_cf.p, (int16_t*)c->ent_cf.p, s));
  HIP_TRY(launch_mcu_code(d, nf, (int)nseg, any_long, (const int16_t*)c->ent_cf.p, optimize != 0,
                          ent_es_tab(c->ent_tab.p), s));
  std::vector<unsigned long long> fl((size_t)nf);
  std::vector<uint32_t> fb((size_t)nf);
  HIP_TRY(hipMemcpyAsync(fl.data(), d.flen, 8 * (size_t)nf, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(fb.data(), d.fbad, 4 * (size_t)nf, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // (h, hdr and frame are this call's objects)
  r->nf = nf;
  r->nseg = (int)nseg;
  r->len.assign((size_t)nf, 0);
  for (int k = 0; k < nf; ++k) {
    if ((long long)fl[(size_t)k] > mcu_capacity(jobs[(size_t)k].f) || fl[(size_t)k] < 4)
      return fail(JDS_EHIP, "writer: file %d reports %llu bytes, outside its bound", k, fl[(size_t)k]);
    r->len[(size_t)k] = fb[(size_t)k] ? 0 : (int64_t)fl[(size_t)k];
  }
  return JDS_OK;
}

// The files at fout (per job; < 0: not written) into out_dev; asynchronous on the context's stream.
static int mcu_emit(jds_ctx* c, const McuRun& r, const std::vector<long long>& fout, uint8_t* out_dev) {
  HIP_TRY(hipMemcpyAsync(r.d.fout, fout.data(), 8 * (size_t)r.nf, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_mcu_emit(r.d, r.nf, r.nseg, out_dev, c->stream));
  return JDS_OK;
}

// One job whose coefficients are in c->ent_cf, to host memory: the writer's
// batch of one, packed at 1, so *out_len is the exact length also where the
// buffer is too small, and a job that is not baseline-codable is JDS_EINVAL.
static int mcu_single(jds_ctx* c, McuJob& job, int32_t optimize, uint8_t* out, int64_t out_cap, int64_t* out_len,
                      const XfSet* xf = nullptr) {
  std::vector<McuJob> jobs(1);
  jobs[0] = std::move(job);
  jds_jpeg_transcode_item it;
  memset(&it, 0, sizeof it);
  int64_t need = 0;
  const CtxMarkScope marks_(c, c->stream);
  const int rc = mcu_write_batch(c, jobs, {0}, optimize, xf, out, out_cap, 0, &it, &need, [](int, const char*) {}, 1);
  if (it.rc) return it.rc;
  if (it.out_len) *out_len = it.out_len;
  return rc;
}

int jds_encode_jpeg(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, int32_t optimize,
                    const uint8_t* prefix, int64_t prefix_len, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  if (!c || !info || !coeffs || !out_len) return fail(JDS_EINVAL, "null argument");
  McuJob job;
  int rc;
  if ((rc = mcu_job_geo(info, 0, &job))) return rc;
  if ((rc = mcu_job_prefix(info, prefix, prefix_len, &job))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nbytes = (size_t)mcu_coeffs(job.f) * sizeof(int16_t);
  HIP_TRY(c->ent_cf.ensure(nbytes));
  HIP_TRY(hipMemcpyAsync(c->ent_cf.p, coeffs, nbytes, hipMemcpyHostToDevice, c->stream));
  return mcu_single(c, job, optimize, out, out_cap, out_len);
}

int jds_jpeg_transcode(jds_ctx* c, const uint8_t* data, int64_t len, int32_t optimize, uint8_t* out, int64_t out_cap,
                       int64_t* out_len, jds_jpeg_info* info) {
  if (!c || !data || !info || !out_len) return fail(JDS_EINVAL, "null argument");
  int rc = jds_jpeg_parse(data, len, info);
  if (rc) return rc;
  McuJob job;
  if ((rc = mcu_job_geo(info, 0, &job))) return rc;
  if ((rc = mcu_job_splice(data, len, &job))) return rc;
  if ((rc = decode_one(c, data, len, info))) return rc;  // (a defective scan: nothing is written)
  return mcu_single(c, job, optimize, out, out_cap, out_len);
}

// One file's transform, settled on the host before anything runs: the
// operation (JDS_XF_AUTO resolved from the spliced prefix), its geometry and
// the prefix, edited unless the operation is none.
struct XfJob {
  int op = JDS_XF_NONE;
  XfPlan plan;
  std::vector<uint8_t> pfx;
};

static inline int64_t xf_align(int64_t entries) { return (entries + 127) & ~(int64_t)127; }

static int xf_prepare(const uint8_t* data, int64_t len, const jds_jpeg_info* info, int32_t op_in, XfJob* x) {
  const int base = op_in & 0xFF;
  if (op_in < 0 || (op_in & ~(0xFF | JDS_XF_TRIM)) || base > JDS_XF_AUTO)
    return fail(JDS_EINVAL, "unknown transform operation 0x%x", (unsigned)op_in);
  McuJob sp;
  int rc = mcu_job_splice(data, len, &sp);
  if (rc) return rc;
  x->pfx = std::move(sp.pfx);
  int64_t pos = -1;
  int big = 0, op = base;
  if (base == JDS_XF_AUTO)
    op = xf_op_of_orientation(xf_exif_orientation(x->pfx.data(), (int64_t)x->pfx.size(), &pos, &big));
  char msg[320];
  if ((rc = xf_plan(info, op, (op_in & JDS_XF_TRIM) != 0, &x->plan, msg, sizeof msg))) return fail(rc, "%s", msg);
  x->op = op;
  if (op == JDS_XF_NONE) return JDS_OK;
  const int e = xf_edit_prefix(x->pfx.data(), (int64_t)x->pfx.size(), x->plan.flags, x->plan.dst.H, x->plan.dst.W);
  if (e == -2) return fail(JDS_ENOTSUP, "DQT: a 16-bit or incomplete table cannot be transposed");
  if (e) return fail(JDS_EINVAL, "header prefix: %s", e == -3 ? "no SOF0 segment" : "not a sequence of marker segments");
  if (pos >= 0) xf_exif_reset(x->pfx.data(), pos, big);
  return JDS_OK;
}

// The writer's job of a transformed file (x.op is not none) whose source planes
// start at src_off of c->ent_cf: the destination planes at *xcur, which moves on
// to the next xf_align'ed place, the record added to xs, the edited prefix.
static int xf_job(XfJob& x, int64_t src_off, int64_t* xcur, XfSet* xs, McuJob* j) {
  const int rc = mcu_job_geo(&x.plan.dst, *xcur, j);
  if (rc) return rc;
  XfFile rec = x.plan.rec;
  for (int cc = 0; cc < 3; ++cc) {
    rec.soff[cc] += src_off;
    rec.doff[cc] += *xcur;
  }
  xs->add(rec);
  *xcur += xf_align(x.plan.dst.coeffs_needed);
  j->pfx = std::move(x.pfx);
  return JDS_OK;
}

// The writer over a batch's jobs, whose coefficients are in c->ent_cf (job k is
// item job_item[k]): its launches, the files packed in job order at multiples
// of `align` into out (jds_jpeg_batch_transcode's contract: 256) with out_off / out_len
// of their items, and rc for a job that is not baseline-codable, of which
// bad(item, message) hears.  Synchronous.
int mcu_write_batch(jds_ctx* c, std::vector<McuJob>& jobs, const std::vector<int>& job_item, int32_t optimize,
                    const XfSet* xf, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                    jds_jpeg_transcode_item* items, int64_t* out_bytes,
                    const std::function<void(int, const char*)>& bad, int64_t align) {
  hipStream_t s = c->stream;
  McuRun r;
  int rc;
  if ((rc = mcu_code(c, jobs, optimize, &r, xf))) return rc;
  std::vector<long long> fout(jobs.size(), -1ll);
  int64_t cur = 0;
  for (size_t k = 0; k < jobs.size(); ++k) {
    const int i = job_item[k];
    if (r.len[k] == 0) {
      items[i].rc = fail(JDS_EINVAL, "%s", MCU_NOT_CODABLE);
      bad(i, MCU_NOT_CODABLE);
      continue;
    }
    fout[k] = cur;
    items[i].out_off = cur;
    items[i].out_len = r.len[k];
    cur = (cur + r.len[k] + align - 1) & -align;
  }
  *out_bytes = cur;
  if (cur > 0 && (!out || out_cap < cur))
    return fail(JDS_EINVAL, "output buffer too small: %lld bytes needed", (long long)cur);
  if (cur > 0) {
    uint8_t* dst = out;
    if (!out_on_device) {
      HIP_TRY(c->ent_out.ensure((size_t)cur));
      dst = (uint8_t*)c->ent_out.p;
    }
    if ((rc = mcu_emit(c, r, fout, dst))) return rc;
    if (!out_on_device)  // file by file: the gaps of the caller's buffer stay as they are
      for (size_t k = 0; k < jobs.size(); ++k)
        if (fout[k] >= 0)
          HIP_TRY(hipMemcpyAsync(out + fout[k], dst + fout[k], (size_t)r.len[k], hipMemcpyDeviceToHost, s));
    kmark(s, "(transcode download)");
    HIP_TRY(hipStreamSynchronize(s));
  }
  return JDS_OK;
}

// jds_jpeg_batch_transcode, and with `xform` jds_jpeg_batch_transform: the same
// launches with per-file transformed records handed to the writer's driver.
static int batch_transcode(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, bool xform,
                           const int32_t* ops, int32_t optimize, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                           jds_jpeg_transcode_item* items, int64_t* out_bytes) {
  if (!c || !out_bytes || (n > 0 && !items)) return fail(JDS_EINVAL, "null argument");
  *out_bytes = 0;
  std::vector<jds_jpeg_batch_item> bi((size_t)(n > 0 ? n : 0));
  BatchPlan bp;
  BaselineFront fe;
  int rc = batch_layout(data, lens, n, bi.data(), bp, fe);
  if (rc) return rc;
  // the transformed planes follow the decoder's in c->ent_cf: sized before the decode fills it
  std::vector<XfJob> xj((size_t)(xform && n > 0 ? n : 0));
  const int64_t xbase = xf_align(bp.coef_entries);
  int64_t xtotal = 0;
  for (int i = 0; xform && i < n; ++i) {
    if (bp.rec_of[(size_t)i] < 0) continue;
    XfJob& x = xj[(size_t)i];
    const int rc1 = xf_prepare(data[i], lens[i], &bp.info[(size_t)i], ops ? ops[i] : JDS_XF_AUTO, &x);
    if (rc1) {  // refused: an item error with the code the file would get alone
      bi[(size_t)i].rc = rc1;
      bp.bad(i, g_err);
      continue;
    }
    bi[(size_t)i].H = x.plan.dst.H;
    bi[(size_t)i].W = x.plan.dst.W;
    if (x.op != JDS_XF_NONE) xtotal += xf_align(x.plan.dst.coeffs_needed);
  }
  if (xtotal) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)(xbase + xtotal)));
  }
  if (!bp.recs.empty() && (rc = batch_run(c, bp, fe, data, lens, nullptr, 0, nullptr, bi.data(), false))) return rc;
  XfSet xs;
  int64_t xcur = xbase;
  return batch_transcode_tail(
      c, bp, bi, n,
      [&](size_t k, int i, McuJob* j) {
        if (xform && xj[(size_t)i].op != JDS_XF_NONE)  // the writer sees the destination planes
          return xf_job(xj[(size_t)i], bp.recs[k].coef_off, &xcur, &xs, j);
        const int r = mcu_job_geo(&bp.info[(size_t)i], bp.recs[k].coef_off, j);
        return r ? r : mcu_job_splice(data[i], lens[i], j);
      },
      &xs, optimize, out, out_cap, out_on_device, items, out_bytes);
}

int batch_transcode_tail(jds_ctx* c, BatchPlan& bp, const std::vector<jds_jpeg_batch_item>& bi, int32_t n,
                         const std::function<int(size_t, int, McuJob*)>& job_of, const XfSet* xf, int32_t optimize,
                         uint8_t* out, int64_t out_cap, int32_t out_on_device, jds_jpeg_transcode_item* items,
                         int64_t* out_bytes) {
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
  // the files that decoded take part in the writer's launches
  std::vector<McuJob> jobs;
  std::vector<int> job_file;
  int rc;
  for (size_t k = 0; k < bp.recs.size(); ++k) {
    const int i = bp.file_of[k];
    if (items[i].status || items[i].rc) continue;
    McuJob j;
    if ((rc = job_of(k, i, &j))) return rc;
    jobs.push_back(std::move(j));
    job_file.push_back(i);
  }
  if (!jobs.empty()) {
    const CtxMarkScope marks_(c, c->stream);
    rc = mcu_write_batch(c, jobs, job_file, optimize, xf && !xf->files.empty() ? xf : nullptr, out, out_cap, out_on_device,
                         items, out_bytes, [&](int i, const char* m) { bp.bad(i, m); });
    if (rc) return rc;
  }
  batch_note(bp);
  return JDS_OK;
}

int jds_jpeg_batch_transcode(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n,
                             int32_t optimize, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                             jds_jpeg_transcode_item* items, int64_t* out_bytes) {
  return batch_transcode(c, data, lens, n, false, nullptr, optimize, out, out_cap, out_on_device, items, out_bytes);
}

// ------------------------------------------------ lossless transforms --
// (DESIGN.md "Lossless transforms"; kernel: jds_xform.hip; host side: jds_xform.hpp)

int jds_jpeg_batch_transform(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n,
                             const int32_t* ops, int32_t optimize, uint8_t* out, int64_t out_cap,
                             int32_t out_on_device, jds_jpeg_transcode_item* items, int64_t* out_bytes) {
  return batch_transcode(c, data, lens, n, true, ops, optimize, out, out_cap, out_on_device, items, out_bytes);
}

int jds_jpeg_transform_info(const uint8_t* data, int64_t len, int32_t op, int32_t* op_out, int64_t* H_out,
                            int64_t* W_out) {
  if (!data || !op_out || !H_out || !W_out) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info info;
  int rc = jds_jpeg_parse(data, len, &info);
  if (rc) return rc;
  XfJob x;
  if ((rc = xf_prepare(data, len, &info, op, &x))) return rc;
  *op_out = x.op;
  *H_out = x.plan.dst.H;
  *W_out = x.plan.dst.W;
  return JDS_OK;
}

int jds_jpeg_transform(jds_ctx* c, const uint8_t* data, int64_t len, int32_t op, int32_t optimize, uint8_t* out,
                       int64_t out_cap, int64_t* out_len, jds_jpeg_info* info) {
  if (!c || !data || !info || !out_len) return fail(JDS_EINVAL, "null argument");
  int rc = jds_jpeg_parse(data, len, info);
  if (rc) return rc;
  XfJob x;
  if ((rc = xf_prepare(data, len, info, op, &x))) return rc;
  McuJob job;
  XfSet xs;
  int64_t xcur = xf_align(info->coeffs_needed);  // the transformed planes follow the decoder's
  if (x.op == JDS_XF_NONE) {  // jds_jpeg_transcode
    if ((rc = mcu_job_geo(info, 0, &job))) return rc;
    job.pfx = std::move(x.pfx);
  } else if ((rc = xf_job(x, 0, &xcur, &xs, &job))) {
    return rc;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)xcur));  // sized before the decode fills the buffer
  if ((rc = decode_one(c, data, len, info))) return rc;  // (a defective scan: nothing is written)
  return mcu_single(c, job, optimize, out, out_cap, out_len, &xs);
}

int jds_selftest_coef_transform_dev(jds_ctx* c, const jds_jpeg_info* info, int32_t op, const int16_t* coeffs,
                                    int16_t* coeffs_out) {
  if (!c || !info || !coeffs || !coeffs_out) return fail(JDS_EINVAL, "null argument");
  const int base_op = op & 0xFF;
  if (op < 0 || (op & ~(0xFF | JDS_XF_TRIM)) || base_op >= JDS_XF_AUTO)
    return fail(JDS_EINVAL, "unknown transform operation 0x%x (an explicit operation is needed)", (unsigned)op);
  XfPlan p;
  char msg[320];
  int rc = xf_plan(info, base_op, (op & JDS_XF_TRIM) != 0, &p, msg, sizeof msg);
  if (rc) return fail(rc, "%s", msg);
  McuFile sf;
  (void)mcu_file_of(info, &sf);  // (xf_plan has checked it)
  const int64_t nsrc = mcu_coeffs(sf), base = xf_align(nsrc), ndst = p.dst.coeffs_needed;
  XfFile rec = p.rec;
  for (int cc = 0; cc < 3; ++cc) rec.doff[cc] += base;
  const size_t o_t = (sizeof(XfFile) + 255) & ~(size_t)255, total = o_t + 4 * (size_t)p.tiles;
  std::vector<char> h(total, 0);  // (the tile table: every tile is record 0's)
  memcpy(h.data(), &rec, sizeof rec);
  hipStream_t s = c->stream;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->mcu_up.ensure(total));
  HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)(base + ndst)));
  int16_t* cf = (int16_t*)c->ent_cf.p;
  HIP_TRY(hipMemcpyAsync(c->mcu_up.p, h.data(), total, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(cf, coeffs, sizeof(int16_t) * (size_t)nsrc, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_coef_xform((const XfFile*)c->mcu_up.p, (const int32_t*)((const char*)c->mcu_up.p + o_t),
                            (long long)p.tiles, cf, cf, s));
  HIP_TRY(hipMemcpyAsync(coeffs_out, cf + base, sizeof(int16_t) * (size_t)ndst, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return JDS_OK;
}

// the host model's result into the caller's buffer
static int mcu_host_result(int wrc, const std::vector<uint8_t>& file, uint8_t* out, int64_t out_cap,
                           int64_t* out_len) {
  if (wrc) return fail(JDS_EINVAL, "%s", MCU_NOT_CODABLE);
  *out_len = (int64_t)file.size();
  if (!out || out_cap < (int64_t)file.size())
    return fail(JDS_EINVAL, "output buffer too small: %lld bytes needed", (long long)file.size());
  memcpy(out, file.data(), file.size());
  return JDS_OK;
}

int jds_selftest_jpeg_transcode(const uint8_t* data, int64_t len, int32_t optimize, uint8_t* out, int64_t out_cap,
                                int64_t* out_len) {
  if (!data || !out_len) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info info;
  int rc = jds_jpeg_parse(data, len, &info);
  if (rc) return rc;
  McuJob job;
  if ((rc = mcu_job_geo(&info, 0, &job))) return rc;
  if ((rc = mcu_job_splice(data, len, &job))) return rc;
  int sb, spg;
  dec_constants(&sb, &spg);
  std::vector<int16_t> cf((size_t)info.coeffs_needed);
  int32_t rounds[3];
  if ((rc = host_decode_parsed(data, &info, sb, cf.data(), info.coeffs_needed, rounds))) return rc;
  McuStdTabs std_tabs;
  mcu_std_tabs(&std_tabs);
  std::vector<uint8_t> file;
  const int wrc = mcu_host_write(job.f, cf.data(), optimize, job.pfx.data(), (int64_t)job.pfx.size(), std_tabs, &file);
  return mcu_host_result(wrc, file, out, out_cap, out_len);
}

int jds_selftest_jpeg_transform(const uint8_t* data, int64_t len, int32_t op, int32_t optimize, uint8_t* out,
                                int64_t out_cap, int64_t* out_len) {
  if (!data || !out_len) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info info;
  int rc = jds_jpeg_parse(data, len, &info);
  if (rc) return rc;
  XfJob x;
  if ((rc = xf_prepare(data, len, &info, op, &x))) return rc;
  McuJob job;
  if ((rc = mcu_job_geo(x.op == JDS_XF_NONE ? &info : &x.plan.dst, 0, &job))) return rc;
  int sb, spg;
  dec_constants(&sb, &spg);
  std::vector<int16_t> cf((size_t)info.coeffs_needed);
  int32_t rounds[3];
  if ((rc = host_decode_parsed(data, &info, sb, cf.data(), info.coeffs_needed, rounds))) return rc;
  if (x.op != JDS_XF_NONE) {
    std::vector<int16_t> dst((size_t)x.plan.dst.coeffs_needed);
    xf_host(x.plan.rec, cf.data(), dst.data());
    cf.swap(dst);
  }
  McuStdTabs std_tabs;
  mcu_std_tabs(&std_tabs);
  std::vector<uint8_t> file;
  const int wrc = mcu_host_write(job.f, cf.data(), optimize, x.pfx.data(), (int64_t)x.pfx.size(), std_tabs, &file);
  return mcu_host_result(wrc, file, out, out_cap, out_len);
}

int jds_selftest_jpeg_encode(const jds_jpeg_info* info, const int16_t* coeffs, int32_t optimize, const uint8_t* prefix,
                             int64_t prefix_len, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  if (!info || !coeffs || !out_len) return fail(JDS_EINVAL, "null argument");
  McuJob job;
  int rc;
  if ((rc = mcu_job_geo(info, 0, &job))) return rc;
  if ((rc = mcu_job_prefix(info, prefix, prefix_len, &job))) return rc;
  McuStdTabs std_tabs;
  mcu_std_tabs(&std_tabs);
  std::vector<uint8_t> file;
  const int wrc = mcu_host_write(job.f, coeffs, optimize, job.pfx.data(), (int64_t)job.pfx.size(), std_tabs, &file);
  return mcu_host_result(wrc, file, out, out_cap, out_len);
}

int jds_selftest_jpeg_hist_dev(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, uint32_t* counts) {
  if (!c || !info || !coeffs || !counts) return fail(JDS_EINVAL, "null argument");
  McuJob job;
  int rc;
  if ((rc = mcu_job_geo(info, 0, &job))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nbytes = (size_t)mcu_coeffs(job.f) * sizeof(int16_t);
  HIP_TRY(c->ent_cf.ensure(nbytes));
  HIP_TRY(hipMemcpyAsync(c->ent_cf.p, coeffs, nbytes, hipMemcpyHostToDevice, c->stream));
  std::vector<McuJob> jobs(1);
  jobs[0] = std::move(job);
  McuRun r;
  if ((rc = mcu_code(c, jobs, 1, &r))) return rc;
  // (the counters open the file's frame)
  HIP_TRY(hipMemcpy(counts, r.d.of, sizeof(uint32_t) * 2 * OPT_BINS, hipMemcpyDeviceToHost));
  return JDS_OK;
}

// --------------------------------------------------- libjpeg encoding --
// (DESIGN.md "libjpeg encoding"; kernel: jds_jpeg_fwd.hip; tile core: jds_jpeg_fwd.hpp)

static int quality_check(int32_t quality, int32_t ss, int64_t H, int64_t W) {
  if (quality < 1 || quality > 100) return fail(JDS_EINVAL, "quality %d outside [1, 100]", (int)quality);
  if (ss != JDS_SS_444 && ss != JDS_SS_422 && ss != JDS_SS_420 && ss != JDS_SS_GRAY)
    return fail(JDS_EINVAL, "unknown subsampling %d (JDS_SS_444, _422, _420 or _GRAY)", (int)ss);
  if (H < 1 || H > 65535) return fail(JDS_EINVAL, "H = %lld outside [1, 65535]", (long long)H);
  if (W < 1 || W > 65535) return fail(JDS_EINVAL, "W = %lld outside [1, 65535]", (long long)W);
  if (H * W > (int64_t)1 << 28) return fail(JDS_EINVAL, "H x W = %lldx%lld: above 2^28 pixels", (long long)H, (long long)W);
  return JDS_OK;
}

int jds_jpeg_quality_info(int32_t quality, int32_t subsampling, int64_t H, int64_t W, jds_jpeg_info* out) {
  if (!out) return fail(JDS_EINVAL, "null argument");
  const int rc = quality_check(quality, subsampling, H, W);
  if (rc) return rc;
  jf_quality_info(quality, subsampling, H, W, out);
  int64_t ny = 0, nc = 0;
  out->reference_grid =
      subsampling != JDS_SS_GRAY && hd_block_counts(H, W, subsampling, &ny, &nc, nullptr, 0) == JDS_OK;
  return JDS_OK;
}

// The launch arguments of an info: jpeg_inv_args' checks of tables and grids.
static int jpeg_fwd_args(const jds_jpeg_info* info, JInvArgs* a) {
  const int rc = jinv_args(info, a);
  if (rc == -1000)
    return fail(JDS_EINVAL, "jpeg forward: %lldx%lld with these grids is not a T.81 geometry of subsampling %d",
                (long long)info->H, (long long)info->W, info->subsampling);
  if (rc < 0) {
    const int c = (-rc - 1) / 64, i = (-rc - 1) % 64;
    return fail(JDS_EINVAL, "qtable[%d][%d] = %g is not an integer in [1, 255]", c, i, info->qtable[c][i]);
  }
  return JDS_OK;
}

static inline size_t rgb_image_bytes(const JInvArgs& a) {
  return (size_t)a.H * (size_t)a.W * (a.ss == JDS_SS_GRAY ? 1u : 3u);
}

int jds_jpeg_forward_dev(jds_ctx* c, const jds_jpeg_info* info, const uint8_t* rgb_dev, int16_t* coeffs_dev,
                         void* stream) {
  if (!info) return fail(JDS_EINVAL, "null argument");
  JInvArgs a;
  int rc;
  if ((rc = jpeg_fwd_args(info, &a))) return rc;
  if (!c || !rgb_dev || !coeffs_dev) return fail(JDS_EINVAL, "null argument");
  if ((uintptr_t)coeffs_dev & 15u) return fail(JDS_EINVAL, "coeffs_dev must be 16-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_jpeg_fwd(a, rgb_dev, coeffs_dev, (hipStream_t)stream));
  return JDS_OK;
}

int jds_selftest_jpeg_forward(const jds_jpeg_info* info, const uint8_t* rgb, int16_t* coeffs_out) {
  if (!info || !rgb || !coeffs_out) return fail(JDS_EINVAL, "null argument");
  JInvArgs a;
  const int rc = jpeg_fwd_args(info, &a);
  if (rc) return rc;
  if ((uintptr_t)coeffs_out & 15u) return fail(JDS_EINVAL, "coeffs_out must be 16-byte aligned");
  jpeg_fwd_host_image(a, rgb, coeffs_out);
  return JDS_OK;
}

int jds_selftest_jpeg_fwd_quant(int32_t q, int32_t n, int32_t* out, int32_t* bound) {
  if (!out || !bound || q < 1 || q > 255 || n < 0) return fail(JDS_EINVAL, "bad argument");
  *bound = JF_CBOUND;
  const uint32_t r = jf_recip(q);
  for (int32_t i = 0; i < n; ++i) {
    out[i] = jf_quant(i, q, r);
    out[n + i] = jf_quant(-i, q, r);
  }
  return JDS_OK;
}

int jds_rgb_to_jpeg(jds_ctx* c, const uint8_t* rgb, int32_t rgb_on_device, int64_t H, int64_t W, int32_t quality,
                    int32_t subsampling, int32_t optimize, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  if (!c || !rgb || !out_len) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info info;
  int rc;
  if ((rc = jds_jpeg_quality_info(quality, subsampling, H, W, &info))) return rc;
  JInvArgs a;
  if ((rc = jpeg_fwd_args(&info, &a))) return rc;
  McuJob job;
  if ((rc = mcu_job_geo(&info, 0, &job))) return rc;
  if ((rc = mcu_job_prefix(&info, nullptr, 0, &job))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->ent_cf.ensure((size_t)info.coeffs_needed * sizeof(int16_t)));
  const uint8_t* src = rgb;
  if (!rgb_on_device) {
    HIP_TRY(c->rgb.ensure(rgb_image_bytes(a)));
    HIP_TRY(hipMemcpyAsync(c->rgb.p, rgb, rgb_image_bytes(a), hipMemcpyHostToDevice, c->stream));
    src = (const uint8_t*)c->rgb.p;
  }
  HIP_TRY(launch_jpeg_fwd(a, src, (int16_t*)c->ent_cf.p, c->stream));
  return mcu_single(c, job, optimize, out, out_cap, out_len);
}

int jds_rgb_batch_to_jpeg(jds_ctx* c, const uint8_t* rgb_base, int32_t rgb_on_device, const jds_rgb_item* items_in,
                          int32_t n, int32_t optimize, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                          jds_jpeg_transcode_item* items, int64_t* out_bytes) {
  if (!c || !out_bytes || n < 0 || (n > 0 && (!items_in || !items || !rgb_base))) return fail(JDS_EINVAL, "null argument");
  *out_bytes = 0;
  BatchBad first;
  auto note = [&](int i, const char* m) { first.bad(i, m); };
  auto finish = [&]() {
    batch_note(first, "image");
    return JDS_OK;
  };
  // the images that take part: records in batch order, coefficients end to end
  std::vector<JInvRec> recs;
  std::vector<McuJob> jobs;
  std::vector<int> job_item;
  int64_t coef_entries = 0, span = 0;
  for (int i = 0; i < n; ++i) {
    const jds_rgb_item& in = items_in[i];
    jds_jpeg_transcode_item& it = items[i];
    memset(&it, 0, sizeof it);
    it.out_off = -1;
    jds_jpeg_info info;
    JInvRec r;
    memset(&r, 0, sizeof r);
    McuJob j;
    int rc = in.rgb_off < 0 ? fail(JDS_EINVAL, "rgb_off %lld", (long long)in.rgb_off)
                            : jds_jpeg_quality_info(in.quality, in.subsampling, in.H, in.W, &info);
    if (rc == JDS_OK) rc = jpeg_fwd_args(&info, &r.a);
    if (rc == JDS_OK) rc = mcu_job_geo(&info, coef_entries, &j);
    if (rc == JDS_OK) rc = mcu_job_prefix(&info, nullptr, 0, &j);
    it.rc = rc;
    if (rc != JDS_OK) {
      note(i, g_err);
      continue;
    }
    it.H = in.H;
    it.W = in.W;
    it.subsampling = in.subsampling;
    it.interleaved = info.interleaved;
    r.coef_off = coef_entries;
    r.rgb_off = in.rgb_off;
    r.st = (int)recs.size();
    coef_entries += info.coeffs_needed;
    const int64_t end = in.rgb_off + (int64_t)rgb_image_bytes(r.a);
    span = end > span ? end : span;
    recs.push_back(r);
    jobs.push_back(std::move(j));
    job_item.push_back(i);
  }
  if (recs.empty()) return finish();
  const int nv = (int)recs.size();
  std::vector<JInvMap> map[JI_MODES];
  if (coef_entries / 64 > 0x7fffffffll || !jinv_batch_maps(recs.data(), nv, map))
    return fail(JDS_ENOTSUP, "batch of %d images: too many blocks or tiles for one set of launches", (int)n);
  int map_off[JI_MODES], nmap[JI_MODES], tiles[JI_MODES], nm = 0;
  for (int m = 0; m < JI_MODES; ++m) {
    map_off[m] = nm;
    nmap[m] = (int)map[m].size() - 1;
    tiles[m] = map[m].back().tile0;
    nm += (int)map[m].size();
  }
  const size_t o_map = (sizeof(JInvRec) * (size_t)nv + 255) & ~(size_t)255, total = o_map + sizeof(JInvMap) * (size_t)nm;
  std::vector<char> h(total, 0);
  memcpy(h.data(), recs.data(), sizeof(JInvRec) * (size_t)nv);
  for (int m = 0; m < JI_MODES; ++m)
    memcpy(h.data() + o_map + sizeof(JInvMap) * (size_t)map_off[m], map[m].data(), sizeof(JInvMap) * map[m].size());
  hipStream_t s = c->stream;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->bat.ensure(total));
  HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)coef_entries));
  const uint8_t* src = rgb_base;
  const CtxMarkScope marks_(c, s);
  // h and the caller's images are copied asynchronously: whichever way this call
  // returns, an error among them, the stream has drained before they go
  struct Settle {
    hipStream_t s;
    ~Settle() { (void)hipStreamSynchronize(s); }
  } const settle_{s};
  if (!rgb_on_device) {  // image by image, at the caller's offsets
    HIP_TRY(c->rgb.ensure((size_t)span));
    for (int k = 0; k < nv; ++k)
      HIP_TRY(hipMemcpyAsync((char*)c->rgb.p + recs[(size_t)k].rgb_off, rgb_base + recs[(size_t)k].rgb_off,
                             rgb_image_bytes(recs[(size_t)k].a), hipMemcpyHostToDevice, s));
    src = (const uint8_t*)c->rgb.p;
  }
  HIP_TRY(hipMemcpyAsync(c->bat.p, h.data(), total, hipMemcpyHostToDevice, s));
  kmark(s, "(batch upload)");
  HIP_TRY(launch_jpeg_fwd_batch((const JInvRec*)c->bat.p, (const JInvMap*)((const char*)c->bat.p + o_map), map_off, nmap,
                                tiles, src, (int16_t*)c->ent_cf.p, s));
  const int rc = mcu_write_batch(c, jobs, job_item, optimize, nullptr, out, out_cap, out_on_device, items, out_bytes, note);
  if (rc) return rc;
  return finish();
}

}  // extern "C"
