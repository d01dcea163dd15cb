// jds_abi_resize.hip — the C-ABI of Pillow resizing (include/jds.h; DESIGN.md
// "Pillow resizing"): the plans, tables and records of a call, their upload and
// the launches of jds_resize.hip.  jds_jpeg_batch_to_tensor is in
// jds_abi_jpeg.hip, beside the decode it drives, and comes here for the resize.
#include <array>
#include <map>

#include "jds_abi.hpp"
#include "jds_resize.hpp"

static int rs_fail(int rc, const char* msg) { return fail(rc == RS_EINVAL ? JDS_EINVAL : JDS_ENOTSUP, "%s", msg); }

// What a call uploads: the tables of its distinct (size, box) pairs, the records
// of the tall images' vertical launch and of the main launch, and their maps.
struct ResizeJob {
  std::vector<int32_t> words;
  std::vector<RsRec> pre, main;
  std::vector<RsMap> pre_map, main_map;
  long long tall_bytes = 0;
};

namespace {

struct Planned {
  bool tall;
  RsRec a, b;  // tall: a the vertical resize into the scratch, b the horizontal one out of it; otherwise a alone
};

// A record that only zeroes its slot.
RsRec zero_rec(long long oh, long long ow) {
  RsRec r;
  memset(&r, 0, sizeof r);
  r.H = r.oh = (int)oh;
  r.W = r.ow = (int)ow;
  r.tw = ow < RS_TW ? (int)ow : RS_TW;
  r.segs = (3 * r.tw + 6) & ~3;
  r.nr = 1;
  r.tiles_x = (r.ow + r.tw - 1) / r.tw;
  r.tiles_y = (r.oh + RS_TH - 1) / RS_TH;
  r.st = -1;
  r.zero = 1;
  return r;
}

int plan_image(long long H, long long W, const float* box, long long oh, long long ow, int flt,
               std::vector<int32_t>& words, Planned* p) {
  char err[300];
  memset(p, 0, sizeof *p);
  int rc;
  if (H >= 1 && W >= 1 && rs_filter_ok(flt) && !rs_check_box(H, W, box, err, sizeof err) && rs_tall(H, W, oh)) {
    const float b1[4] = {0.0f, box[1], (float)W, box[3]}, b2[4] = {box[0], 0.0f, box[2], (float)oh};
    p->tall = true;
    if ((rc = rs_plan(H, W, b1, oh, W, flt, words, &p->a, nullptr, err, sizeof err))) return rs_fail(rc, err);
    if ((rc = rs_plan(oh, W, b2, oh, ow, flt, words, &p->b, nullptr, err, sizeof err))) return rs_fail(rc, err);
    return JDS_OK;
  }
  if ((rc = rs_plan(H, W, box, oh, ow, flt, words, &p->a, nullptr, err, sizeof err))) return rs_fail(rc, err);
  return JDS_OK;
}

bool add_to_map(std::vector<RsMap>& map, long long* tiles, const RsRec& r, int rec) {
  map.push_back(RsMap{(int)*tiles, rec});
  *tiles += (long long)r.tiles_x * r.tiles_y;
  return *tiles <= 0x7fffffffll;
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

int ensure_host(jds_ctx* c, size_t bytes) {
  if (bytes <= c->rsz_host_cap) return JDS_OK;
  if (c->rsz_host) (void)hipHostFree(c->rsz_host);
  c->rsz_host = nullptr;
  c->rsz_host_cap = 0;
  HIP_TRY(hipHostMalloc(&c->rsz_host, bytes, hipHostMallocDefault));
  c->rsz_host_cap = bytes;
  return JDS_OK;
}

// What has been queued on s so far has run: the staging and the tables may be rewritten.
int wait_done(jds_ctx* c, hipStream_t s) {
  if (!c->rsz_ev) HIP_TRY(hipEventCreateWithFlags(&c->rsz_ev, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c->rsz_ev, s));
  HIP_TRY(hipEventSynchronize(c->rsz_ev));
  return JDS_OK;
}

}  // namespace

void resize_ctx_release(jds_ctx* c) {
  c->rsz_tab.release();
  c->rsz_tall.release();
  c->rsz_src.release();
  if (c->rsz_host) (void)hipHostFree(c->rsz_host);
  c->rsz_host = nullptr;
  c->rsz_host_cap = 0;
  if (c->rsz_ev) (void)hipEventDestroy(c->rsz_ev);
  c->rsz_ev = nullptr;
}

void resize_job_free(ResizeJob* j) { delete j; }

int resize_job_build(const ResizeSrc* items, int n, long long oh, long long ow, int flt, ResizeJob** out) {
  *out = nullptr;
  if (!rs_filter_ok(flt))
    return fail(JDS_EINVAL, "unknown resampling filter %d: 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING", flt);
  if (oh < 1 || ow < 1) return fail(JDS_EINVAL, "bad size: %lld x %lld (width x height)", ow, oh);
  if (oh > 0x7fffffffll / 3 || ow > 0x7fffffffll / 3 || oh * ow * 3 > 0x7fffffffll)
    return fail(JDS_ENOTSUP, "image too large: more than 2^31 - 1 bytes");
  ResizeJob* j = new ResizeJob();
  std::map<std::array<int64_t, 4>, Planned> seen;  // images of one size and box share their tables
  long long pre_tiles = 0, main_tiles = 0;
  const long long slot = oh * ow * 3;
  bool over = false;
  for (int i = 0; i < n; ++i) {
    const ResizeSrc& it = items[i];
    RsRec r;
    if (it.zero) {
      r = zero_rec(oh, ow);
    } else {
      const float full[4] = {0.0f, 0.0f, (float)it.W, (float)it.H};
      const float* box = it.has_box ? it.box : full;
      int32_t bits[4];
      memcpy(bits, box, sizeof bits);
      const std::array<int64_t, 4> key = {it.H, it.W, ((int64_t)bits[0] << 32) | (uint32_t)bits[1],
                                          ((int64_t)bits[2] << 32) | (uint32_t)bits[3]};
      auto f = seen.find(key);
      if (f == seen.end()) {
        Planned p;
        const int rc = it.off < 0 ? fail(JDS_EINVAL, "negative offset")
                                  : plan_image(it.H, it.W, box, oh, ow, flt, j->words, &p);
        if (rc) {
          char m[400];
          snprintf(m, sizeof m, "%s", g_err);
          delete j;
          return fail(rc, "image %d: %s", i, m);
        }
        f = seen.emplace(key, p).first;
      }
      const Planned& p = f->second;
      r = p.tall ? p.b : p.a;
      r.src_off = it.off;
      r.st = it.st;
      if (p.tall) {
        RsRec a = p.a;
        a.src_off = it.off;
        a.dst_off = j->tall_bytes;
        a.dst_sel = 1;
        a.st = it.st;
        r.src_off = j->tall_bytes;
        r.src_sel = 1;
        j->tall_bytes += ((long long)a.oh * a.ow * 3 + 255) / 256 * 256;
        if (!add_to_map(j->pre_map, &pre_tiles, a, (int)j->pre.size())) over = true;
        j->pre.push_back(a);
      }
    }
    r.dst_off = slot * i;
    if (!add_to_map(j->main_map, &main_tiles, r, i)) over = true;
    j->main.push_back(r);
    if (over) {
      delete j;
      return fail(JDS_ENOTSUP, "batch of %d images: too many tiles for one launch", n);
    }
  }
  j->pre_map.push_back(RsMap{(int)pre_tiles, -1});
  j->main_map.push_back(RsMap{(int)main_tiles, -1});
  *out = j;
  return JDS_OK;
}

int resize_job_enqueue(jds_ctx* c, ResizeJob* j, const uint8_t* src_dev, const uint32_t* status_dev, uint8_t* out_dev,
                       hipStream_t s, bool wait) {
  if (j->main.empty()) return JDS_OK;
  const size_t o_words = 0, o_pre = up256(sizeof(int32_t) * j->words.size()),
               o_pmap = up256(o_pre + sizeof(RsRec) * j->pre.size()),
               o_main = up256(o_pmap + sizeof(RsMap) * j->pre_map.size()),
               o_mmap = up256(o_main + sizeof(RsRec) * j->main.size()),
               total = up256(o_mmap + sizeof(RsMap) * j->main_map.size());
  int rc;
  if ((rc = ensure_host(c, total))) return rc;
  HIP_TRY(c->rsz_tab.ensure(total));
  HIP_TRY(c->rsz_tall.ensure((size_t)j->tall_bytes));
  char* h = (char*)c->rsz_host;
  if (!j->words.empty()) memcpy(h + o_words, j->words.data(), sizeof(int32_t) * j->words.size());
  if (!j->pre.empty()) memcpy(h + o_pre, j->pre.data(), sizeof(RsRec) * j->pre.size());
  memcpy(h + o_pmap, j->pre_map.data(), sizeof(RsMap) * j->pre_map.size());
  memcpy(h + o_main, j->main.data(), sizeof(RsRec) * j->main.size());
  memcpy(h + o_mmap, j->main_map.data(), sizeof(RsMap) * j->main_map.size());
  char* dv = (char*)c->rsz_tab.p;
  HIP_TRY(hipMemcpyAsync(dv, h, total, hipMemcpyHostToDevice, s));
  kmark(s, "(resize upload)");
  const int32_t* tabs = (const int32_t*)(dv + o_words);
  uint8_t* tall = (uint8_t*)c->rsz_tall.p;
  HIP_TRY(launch_resize_batch((const RsRec*)(dv + o_pre), (const RsMap*)(dv + o_pmap), (int)j->pre.size(),
                              j->pre_map.back().tile0, status_dev, tabs, src_dev, nullptr, nullptr, tall, s));
  HIP_TRY(launch_resize_batch((const RsRec*)(dv + o_main), (const RsMap*)(dv + o_mmap), (int)j->main.size(),
                              j->main_map.back().tile0, status_dev, tabs, src_dev, tall, out_dev, nullptr, s));
  return wait ? wait_done(c, s) : JDS_OK;
}

extern "C" {

int jds_resize_info(int32_t* tile_h, int32_t* tile_w, int32_t* max_taps) {
  if (!tile_h || !tile_w || !max_taps) return fail(JDS_EINVAL, "null argument");
  *tile_h = RS_TH;
  *tile_w = RS_TW;
  *max_taps = RS_MAX_TAPS;
  return JDS_OK;
}

int jds_selftest_resize_coeffs(int32_t in_size, float in0, float in1, int32_t out_size, int32_t resample,
                               int32_t* ksize, int32_t* bounds, int32_t* taps, int64_t cap) {
  if (!ksize || !bounds || !taps) return fail(JDS_EINVAL, "null argument");
  if (!rs_filter_ok(resample)) return fail(JDS_EINVAL, "unknown resampling filter %d", (int)resample);
  if (in_size < 1 || out_size < 1 || !(in0 < in1)) return fail(JDS_EINVAL, "bad axis");
  const double ks = rs_ksize(in0, in1, out_size, resample);
  if (ks * out_size > 1e9) return fail(JDS_ENOTSUP, "table too large");
  *ksize = (int32_t)ks;
  if ((int64_t)ks * out_size > cap)
    return fail(JDS_EINVAL, "taps: %lld entries needed", (long long)((int64_t)ks * out_size));
  RsAxisTab t;
  rs_coeffs(in_size, in0, in1, out_size, resample, &t);
  memcpy(bounds, t.bounds.data(), sizeof(int32_t) * t.bounds.size());
  memcpy(taps, t.taps.data(), sizeof(int32_t) * t.taps.size());
  return JDS_OK;
}

int jds_selftest_resize(const uint8_t* rgb, int64_t H, int64_t W, const float* box, int64_t out_h, int64_t out_w,
                        int32_t resample, uint8_t* out, int64_t* worst) {
  if (!rgb || !out) return fail(JDS_EINVAL, "null argument");
  char err[300];
  long long w = 0;
  const int rc = rs_host_resize(rgb, H, W, box, out_h, out_w, resample, out, &w, err, sizeof err);
  if (rc) return rs_fail(rc, err);
  if (worst) *worst = w;
  return JDS_OK;
}

int jds_rgb_resize(jds_ctx* c, const uint8_t* rgb, int32_t rgb_on_device, int64_t H, int64_t W, const float* box_in,
                   int64_t out_h, int64_t out_w, int32_t resample, uint8_t* out, int32_t out_on_device) {
  if (!c || !rgb || !out) return fail(JDS_EINVAL, "null argument");
  const float full[4] = {0.0f, 0.0f, (float)W, (float)H};
  const float* box = box_in ? box_in : full;
  std::vector<int32_t> words;
  Planned p;
  int rc;
  if (out_h < 1 || out_w < 1 || H < 1 || W < 1)
    return fail(JDS_EINVAL, "bad size: %lld x %lld to %lld x %lld (width x height)", (long long)W, (long long)H,
                (long long)out_w, (long long)out_h);
  if ((rc = plan_image(H, W, box, out_h, out_w, resample, words, &p))) return rc;
  p.a.st = p.b.st = -1;
  hipStream_t s = c->stream;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nin = (size_t)H * (size_t)W * 3, nout = (size_t)out_h * (size_t)out_w * 3,
               nw = up256(sizeof(int32_t) * (words.size() + 1));
  if ((rc = ensure_host(c, nw))) return rc;
  HIP_TRY(c->rsz_tab.ensure(nw));
  const uint8_t* src = rgb;
  uint8_t* dst = out;
  if (!rgb_on_device) {
    HIP_TRY(c->rsz_src.ensure(nin));
    HIP_TRY(hipMemcpyAsync(c->rsz_src.p, rgb, nin, hipMemcpyHostToDevice, s));
    src = (const uint8_t*)c->rsz_src.p;
  }
  if (!out_on_device) {
    HIP_TRY(c->out.ensure(nout));
    dst = (uint8_t*)c->out.p;
  }
  if (!words.empty()) memcpy(c->rsz_host, words.data(), sizeof(int32_t) * words.size());
  HIP_TRY(hipMemcpyAsync(c->rsz_tab.p, c->rsz_host, nw, hipMemcpyHostToDevice, s));
  const int32_t* tabs = (const int32_t*)c->rsz_tab.p;
  if (p.tall) {
    HIP_TRY(c->rsz_tall.ensure((size_t)p.a.oh * (size_t)p.a.ow * 3));
    HIP_TRY(launch_resize(p.a, tabs, src, (uint8_t*)c->rsz_tall.p, s));
    HIP_TRY(launch_resize(p.b, tabs, (const uint8_t*)c->rsz_tall.p, dst, s));
  } else {
    HIP_TRY(launch_resize(p.a, tabs, src, dst, s));
  }
  if (!out_on_device) HIP_TRY(hipMemcpyAsync(out, dst, nout, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return JDS_OK;
}

int jds_rgb_batch_resize(jds_ctx* c, const uint8_t* rgb_base_dev, const jds_resize_item* items, int32_t n,
                         int64_t out_h, int64_t out_w, int32_t resample, uint8_t* out_dev, void* stream) {
  if (!c || n < 0 || (n > 0 && (!rgb_base_dev || !items || !out_dev))) return fail(JDS_EINVAL, "null argument");
  std::vector<ResizeSrc> src((size_t)n);
  for (int i = 0; i < n; ++i) {
    ResizeSrc& r = src[(size_t)i];
    memset(&r, 0, sizeof r);
    r.off = items[i].rgb_off;
    r.H = items[i].H;
    r.W = items[i].W;
    r.st = -1;
    r.has_box = items[i].has_box != 0;
    memcpy(r.box, items[i].box, sizeof r.box);
  }
  ResizeJob* job = nullptr;
  int rc = resize_job_build(src.data(), n, out_h, out_w, resample, &job);
  if (rc) return rc;
  if (hipSetDevice(c->device) != hipSuccess) {
    resize_job_free(job);
    return fail(JDS_EHIP, "hipSetDevice");
  }
  {
    const CtxMarkScope marks_(c, (hipStream_t)stream);
    rc = resize_job_enqueue(c, job, rgb_base_dev, nullptr, out_dev, (hipStream_t)stream, true);
  }
  resize_job_free(job);
  return rc;
}

}  // extern "C"
